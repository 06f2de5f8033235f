"""How much of the hand-scheduled body of the tuned LAv2 kernel (FS_FAST_LOOP_FDU, csrc/scaled_runs.hpp) runs in its add-free form,
by workload: the statement's wave-steps, the share the ND form carried (word 30, NDZ bodies included) and the share that ran
without the dz add as well (NDZ, word 35), the ND verdicts that failed (each repeats its run in the full form), the full-form wave-steps
taken while a wave was backing off from a refused entry vote or a failed verdict (word 36) and those among them whose entry vote would
have passed (word 37: what the back-off policy leaves on the table), the NDZ wave-steps in bodies that the one-term bound
(dc riding on dz's term, the bound before dc got a term of its own) would have refused (word 38: what the second term buys), and the counting instantiation's replay of every accepted add-free
invocation in the full form (mismatches must be 0).
Usage: python tools/add_free_probe.py [view width height [cpu|cpu_gpustage]] ...   (default: View 5 at 64x36 and at 3840x2160)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fractalshark_amd import GPURenderer, LAV2_FULL, PARITY_CPU, PARITY_CPU_GPUSTAGE, T_HDR32, inputs  # noqa: E402

args = sys.argv[1:]
jobs = []
while args:
    n = 4 if len(args) >= 4 and args[3] in ("cpu", "cpu_gpustage") else 3
    jobs.append((int(args[0]), int(args[1]), int(args[2]), args[3] if n == 4 else "cpu"))
    args = args[n:]
if not jobs:
    jobs = [(5, 64, 36, "cpu"), (5, 3840, 2160, "cpu")]
r = GPURenderer(0)
for view, w, h, parity in jobs:
    v = inputs.View.builtin(view, w, h, antialiasing=1)
    o = inputs.Orbit(v)
    la = inputs.LATable(o)
    co = [(float(c["m"]), int(c["e"])) for c in v.coords_perturb(o)]
    par = PARITY_CPU if parity == "cpu" else PARITY_CPU_GPUSTAGE
    assert r.InitializeMemory(w, h, 1, None, 0, 0, 0, False) == 0
    assert r.InitializePerturb(1, o, 0, None, la) == 0
    r.enable_step_count(True)
    assert r.RenderPerturbLAv2(None, None, None, *co, v.num_iterations, T=T_HDR32, Mode=LAV2_FULL, parity=par) == 0
    assert r.SyncComputeStream() == 0
    st = r.read_step_count()
    raw = (C.c_uint64 * 40)()
    assert r._lib.fs_read_stats_raw(r._h, raw, 40) == 0
    r.enable_step_count(False)
    statement = 4 * raw[8]
    print(json.dumps({"view": view, "size": "%dx%d" % (w, h), "parity": parity,
                      "perturb_lane_steps": st["perturb_steps"],
                      "statement_wave_steps": statement,
                      "nd_wave_steps": raw[30], "nd_share_of_statement": round(raw[30] / max(1, statement), 4),
                      "ndz_wave_steps": raw[35], "ndz_share_of_statement": round(raw[35] / max(1, statement), 4),
                      "ndz_share_of_nd": round(raw[35] / max(1, raw[30]), 4),
                      "nd_verdicts_failed": raw[32],
                      "full_form_wave_steps": statement - raw[30],
                      "backed_off_full_form_wave_steps": raw[36], "backed_off_with_passing_vote": raw[37],
                      "ndz_wave_steps_owed_to_the_dc_term": raw[38],
                      "predicted_valu_instructions_saved_by_the_dc_term": 1.25 * raw[38],
                      "invocations_replayed": raw[34], "replay_mismatches": raw[33],
                      "predicted_valu_instructions_saved_by_nd": raw[30],
                      "predicted_valu_instructions_saved_by_ndz": 1.25 * raw[35]}), flush=True)
r.close()
