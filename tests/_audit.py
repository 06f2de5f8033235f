"""The rule of fs_exact_audit restated with numpy -- test infrastructure shared by tests/test_exact_audit_cpu.py and
tests/test_gpu_exact_audit.py.  `expected` derives every field of the record from per-sample arrays; `same_record` compares a
_capi.AuditResult (or anything with the same attributes) with it, field by field, integers only."""
import numpy as np

MAX_LEVELS, MAX_OFFENDERS = 8, 16


def expected(frame_values, exact, stable, cap):
    """frame_values, exact: int[n]; stable: bool[n, k]; the record as a dict (per-level lists of length k, offenders as tuples
    (sample, stable_bits, frame_value, exact_value))."""
    frame_values, exact = np.asarray(frame_values, np.int64), np.asarray(exact, np.int64)
    stable = np.asarray(stable, bool).reshape(len(exact), -1)
    n, k = stable.shape
    differ, capped = frame_values != exact, exact == cap
    diff = np.abs(frame_values - exact)
    bits = (stable.astype(np.int64) << np.arange(k)[None, :]).sum(axis=1) if k else np.zeros(n, np.int64)
    first = np.flatnonzero(differ)[:MAX_OFFENDERS]
    return {
        "n_samples": n, "n_levels": k, "n_equal": int((~differ).sum()), "n_differ": int(differ.sum()), "n_capped": int(capped.sum()),
        "n_offenders": len(first),
        "stable": [int(stable[:, j].sum()) for j in range(k)],
        "stable_differ": [int((stable[:, j] & differ).sum()) for j in range(k)],
        "stable_capped": [int((stable[:, j] & capped).sum()) for j in range(k)],
        "max_abs_diff": [int(diff[stable[:, j] & differ].max()) if (stable[:, j] & differ).any() else 0 for j in range(k)],
        "offenders": [(int(i), int(bits[i]), int(frame_values[i]), int(exact[i])) for i in first],
        "stable_bits": bits,
    }


def record_dict(res):
    """A _capi.AuditResult as the dict `expected` makes (whole arrays: what lies beyond n_levels / n_offenders must be zero)."""
    k, m = res.n_levels, res.n_offenders
    for name in ("stable", "stable_differ", "stable_capped", "max_abs_diff"):
        assert not any(getattr(res, name)[k:]), name
    for o in res.offenders[m:]:
        assert (o.sample, o.stable_bits, o.frame_value, o.exact_value) == (0, 0, 0, 0)
    return {
        "n_samples": res.n_samples, "n_levels": k, "n_equal": res.n_equal, "n_differ": res.n_differ, "n_capped": res.n_capped,
        "n_offenders": m,
        "stable": list(res.stable[:k]), "stable_differ": list(res.stable_differ[:k]), "stable_capped": list(res.stable_capped[:k]),
        "max_abs_diff": list(res.max_abs_diff[:k]),
        "offenders": [(o.sample, o.stable_bits, o.frame_value, o.exact_value) for o in res.offenders[:m]],
    }


def same_record(res, want):
    got = record_dict(res)
    for key, v in got.items():
        assert v == want[key], (key, v, want[key])
