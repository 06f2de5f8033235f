"""features.pt_grid's records through fs_feature_eval: the period search of a dense grid of a deep view in one call, bit for bit
the CPU checker's (tests/feature/feature_ref.cpp) -- a view where the Direct period map is one constant."""
import numpy as np
import pytest

from fractalshark_amd import T_HDR32, features
from test_feature_finder_cpu import checker_evaluator
from test_feature_map_cpu import view5
from test_gpu_feature_finder import renderer_for

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny", [(1, 1), (65, 1), (24, 13)])  # one lane; a full wave and one lane; four waves and 56 lanes
def test_pt_grid_through_feature_eval_equals_the_checker(nx, ny):
    v, ob = view5()
    cap = 1 << 16
    rin, rad = features.pt_grid(v, ob, nx, ny)
    gpu, cpu = np.zeros(len(rin), features.FEATURE_OUT_HDR32), np.zeros(len(rin), features.FEATURE_OUT_HDR32)
    r = renderer_for(ob)
    assert r.FeatureEval(T_HDR32, 4, features.FIND, rad, cap, rin, gpu) == 0
    r.close()
    checker_evaluator(ob, 4, threads=16)(features.FIND, rad, cap, rin, cpu)
    assert gpu.tobytes() == cpu.tobytes(), np.nonzero(gpu != cpu)[0][:8]
    if (nx, ny) == (24, 13):
        periods = np.where(gpu["status"] == features.OK, gpu["period"], 0)
        assert periods.any() and len(np.unique(rin["c"])) == 1  # Direct would see one point; PT tells 312 apart
