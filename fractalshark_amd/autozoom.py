"""The AutoZoomer's loop (AutoZoomer::Run, AutoZoomer.cpp:30-437) with the frame analysis on the GPU.

The reference renders a frame, scans the iteration array on one CPU thread for the next target (Default: weighted mean position;
Max: first pixel at the largest count; FilamentTip: best-scoring tip), recentres on it and starts again.  Here the scan is
fs_autozoom_pick next to the buffer the render kernels wrote -- nothing but the record comes back -- and the next view is
computed by libfsinputs at the view's precision.
"""
DEFAULT, MAX, FILAMENT_TIP = 0, 1, 2  # FS_AUTOZOOM_* heuristics
MOVE, MOVE_THEN_STOP, FLAT, NO_TARGET = 0, 1, 2, 3  # FS_AUTOZOOM_* status
DIVISOR = {DEFAULT: 3, MAX: 32, FILAMENT_TIP: 8}  # AutoZoomer.cpp:36-45


def pick(renderer, heuristic, n_iterations):
    """The target of the renderer's current frame: a _capi.AutozoomResult (fs_autozoom_result, include/fs_layout.h)."""
    err, res = renderer.AutozoomPick(heuristic, n_iterations)
    if err:
        raise RuntimeError("fs_autozoom_pick failed: %d (%s)" % (err, renderer.ConvertErrorToString(err)))
    return res


def next_view(view, picked):
    """The view the AutoZoomer recentres to after `picked` (status MOVE or MOVE_THEN_STOP)."""
    if picked.status not in (MOVE, MOVE_THEN_STOP):
        raise ValueError("the pick does not move (status %d)" % picked.status)
    return view.autozoom_next(picked.target_x, picked.target_y, DIVISOR[int(picked.heuristic)])


def zoom(renderer, view, heuristic, render, max_steps):
    """Generator: render(renderer, view) -> pick -> next view, up to max_steps times or until a pick says stop.  `render` is
    the caller's: it leaves the view's frame in the renderer's iteration buffer (a direct or a perturbation render, on the
    compute stream).  Yields (view, pick, next view or None) per step; the loop ends after a step whose pick does not move, or
    moves and stops (the reference's num_at_max > 500)."""
    for _ in range(int(max_steps)):
        render(renderer, view)
        picked = pick(renderer, heuristic, view.num_iterations)
        if picked.status in (FLAT, NO_TARGET):
            yield view, picked, None
            return
        nv = next_view(view, picked)
        yield view, picked, nv
        if picked.status == MOVE_THEN_STOP:
            return
        view = nv


__all__ = ["DEFAULT", "MAX", "FILAMENT_TIP", "MOVE", "MOVE_THEN_STOP", "FLAT", "NO_TARGET", "DIVISOR", "pick", "next_view",
           "zoom"]
