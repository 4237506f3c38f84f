"""okge_adam_multi (adam_prologue_kernel + adam_multi_kernel, csrc/okge_adam.hip) through the C ABI.  Its element update is
okge_adam_step's, so the yardstick is okge_adam_step itself, run on copies of the same tensors in pairs: p, exp_avg, exp_avg_sq, t
and the cleared gradients must come out BIT-EQUAL -- one to four tensors of mixed sizes, weight decay present and absent, a cold
and a warm state, a shared state, one tensor above the launcher's grid cap.  At two shapes the result is also held to adam_caps
against the float64 restatement, as test_adam_shapes.py does.  With a touched-row map the twin is okge_adam_step on a copy whose
unstamped gradient rows are zero, while the tensor under test holds NaN there: the NaNs must survive bit for bit (neither read
nor cleared), stamped rows are cleared, the map is left alone.  Every tensor sits in a sentinel-filled buffer whose guard words
must survive."""
import numpy as np
import pytest
import torch

import adam_reference as A
from test_adam_shapes import BETAS, EPS, LR, Seg, check_against_float64, make_seg
from test_adam_shapes import launch as launch_step
from test_optim_shapes import CAP, NAN_BITS, Guarded, same_bits

pytestmark = pytest.mark.gpu

STAMP = 7
SIZES = (0, 1, 3, 255, 1027, 262_147)
N_BIG = CAP + 259


@pytest.fixture(scope="module")
def hp(okge_lib):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


def launch_multi(hp, segs, wd, maps=None):
    """maps: per tensor None or (Guarded byte map, row_len, stamp)"""
    from open_knowledge_graph_embeddings_amd import _native as N
    arr = (N.AdamMultiTensor * len(segs))()
    for k, (a, sg) in enumerate(zip(arr, segs)):
        a.p, a.g, a.exp_avg, a.exp_avg_sq, a.state, a.n = sg.p.ptr(), sg.g.ptr(), sg.m.ptr(), sg.v.ptr(), sg.state.ptr(), sg.n
        if maps is not None and maps[k] is not None:
            a.row_touched, a.row_len, a.touched_stamp = maps[k][0].ptr(), int(maps[k][1]), int(maps[k][2])
    return int(hp.lib.okge_adam_multi(arr, len(segs), LR, BETAS[0], BETAS[1], EPS, wd, hp._stream()))


def twin_of(sg, g=None):
    return Seg(sg.h[0], sg.h[1] if g is None else g, sg.h[2], sg.h[3], sg.t)


def step_in_pairs(hp, twins, wd):
    """okge_adam_step over the twins, two per call, gradients cleared"""
    for i in range(0, len(twins), 2):
        assert launch_step(hp, twins[i:i + 2], wd, 1) == 0, hp.lib.okge_last_error()


def assert_same(case, segs, twins, cleared=True):
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(segs, twins)):
        for name in ("p", "m", "v"):
            assert same_bits(getattr(a, name).v, getattr(b, name).v), (case, k, name)
        assert torch.equal(a.state.v, b.state.v), (case, k, "state", a.state.np(), b.state.np())
        if cleared:
            assert not bool(a.g.v.any()) and not bool(torch.signbit(a.g.v).any()), (case, k, "gradient not cleared to +0")
        assert a.intact() and b.intact(), (case, k, "guard words overwritten")


MIXES = [(1027,), (0,), (0, 262_147), (3, 1), (255, 3, 1027), (262_147, 0, 1), (262_147, 1, 0, 255), (3, 1027, 255, 262_147), (1, 1, 1, 1)]


@pytest.mark.parametrize("warm", [False, True], ids=["cold-t0", "warm-t1000"])
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("ns", MIXES, ids=lambda ns: "-".join(map(str, ns)))
def test_without_maps_is_bit_equal_to_adam_step(hp, ns, wd, warm):
    assert set(n for mix in MIXES for n in mix) == set(SIZES)
    t0 = 1000 if warm else 0
    segs = [make_seg(n, 20 + k, warm, t0) for k, n in enumerate(ns)]
    twins = [twin_of(sg) for sg in segs]
    for step in range(2):                                      # the second step starts from the first one's moments and a zero gradient
        assert launch_multi(hp, segs, wd) == 0, hp.lib.okge_last_error()
        step_in_pairs(hp, twins, wd)
        assert_same("mix-%s-step%d" % (ns, step), segs, twins)
        assert all(int(sg.state.np()[0]) == t0 + step + 1 for sg in segs)


@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("ns", [(1027, 3), (255, 262_147, 1)], ids=["1027-3", "255-262147-1"])
def test_against_float64(hp, ns, wd):
    segs = [make_seg(n, 30 + k, True, 999) for k, n in enumerate(ns)]
    assert launch_multi(hp, segs, wd) == 0, hp.lib.okge_last_error()
    torch.cuda.synchronize()
    for k, sg in enumerate(segs):
        check_against_float64("multi-%s-wd%g" % (ns, wd), "t%d" % k, [sg.p.np(), sg.m.np(), sg.v.np()], *sg.h, 1000, wd)
        assert int(sg.state.np()[0]) == 1000 and sg.intact()


def test_shared_state_advances_once(hp):
    """tensors 0 and 2 hand over ONE state, tensor 1 its own: each distinct state advances by one per call"""
    segs = [make_seg(1027, 40, True, 6), make_seg(255, 41, True, 2), make_seg(3, 42, True, 6)]
    segs[2].state = segs[0].state
    twins = [twin_of(sg) for sg in segs]
    twins[2].state = twins[0].state
    for step in range(2):
        assert launch_multi(hp, segs, 1e-2) == 0, hp.lib.okge_last_error()
        assert launch_step(hp, [twins[0], twins[2]], 1e-2, 1) == 0 and launch_step(hp, [twins[1]], 1e-2, 1) == 0
        assert_same("shared-step%d" % step, segs, twins)
    assert int(segs[0].state.np()[0]) == 8 and int(segs[1].state.np()[0]) == 4


def test_above_the_grid_cap(hp):
    """16 777 216 + 259 floats: one full pass of the grid-stride loop, a partial second pass and a tail of 3, next to a short tensor"""
    src = A.sweep_inputs(N_BIG, 5, True)
    segs = [make_seg(N_BIG, 0, True, 1, src=src), make_seg(7, 43, True, 1)]
    twins = [twin_of(sg) for sg in segs]
    assert launch_multi(hp, segs, 1e-2) == 0, hp.lib.okge_last_error()
    step_in_pairs(hp, twins, 1e-2)
    assert_same("big", segs, twins)


# ---- touched-row maps -------------------------------------------------------------------------------------------------------------
def stamp_pattern(kind, rows, rng):
    m = np.zeros(rows, np.uint8)
    if kind == "all":
        m[:] = STAMP
    elif kind == "every-third":
        m[::3] = STAMP
    elif kind == "first-and-last":
        m[0] = m[-1] = STAMP
    elif kind == "stale":                                      # stamps of other updates, and a few rows of this one
        m[:] = rng.choice(np.array([STAMP - 1, STAMP + 1, 255, 1], np.uint8), rows)
        m[rng.random(rows) < 0.3] = STAMP
    return m


def mapped_pair(rows, row_len, kind, seed, t0=3):
    """(tensor under test: NaN in the gradient rows the map does not stamp; its twin: zeros there; the map; the live mask)"""
    n = rows * row_len
    rng = np.random.default_rng([70, rows, row_len, seed])
    sg = make_seg(n, seed, True, t0)
    m = stamp_pattern(kind, rows, rng)
    live = np.repeat(m == STAMP, row_len)
    twin = twin_of(sg, np.where(live, sg.h[1], np.float32(0)))
    nan = torch.full((n,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    live_dev = torch.from_numpy(live).cuda()
    sg.g.v.copy_(torch.where(live_dev, sg.g.v, nan))
    return sg, twin, Guarded(m), m, live_dev, nan


def check_mapped(case, sg, map_dev, m, live_dev, nan):
    want_g = torch.where(live_dev, torch.zeros_like(nan), nan)
    assert same_bits(sg.g.v, want_g), (case, "stamped gradient rows must be +0, the NaNs of the other rows untouched")
    assert map_dev.intact() and np.array_equal(map_dev.np(), m), (case, "the map is left as it was")


@pytest.mark.parametrize("row_len", [4, 8, 200, 512])
def test_with_maps_is_bit_equal_to_adam_step_on_zeroed_rows(hp, row_len):
    """row lengths 4, 8 and 512 take the shift, 200 the division; 63 / 64 / 65 rows around a wave's worth"""
    for rows in (1, 63, 64, 65, 1000):
        for i, kind in enumerate(("none", "all", "every-third", "first-and-last", "stale")):
            wd = (0.0, 1e-2)[(rows + i) % 2]
            case = "map-r%d-l%d-%s-wd%g" % (rows, row_len, kind, wd)
            sg, twin, map_dev, m, live_dev, nan = mapped_pair(rows, row_len, kind, 50 + i)
            assert launch_multi(hp, [sg], wd, [(map_dev, row_len, STAMP)]) == 0, (case, hp.lib.okge_last_error())
            assert launch_step(hp, [twin], wd, 1) == 0
            assert_same(case, [sg], [twin], cleared=False)
            check_mapped(case, sg, map_dev, m, live_dev, nan)


def test_mapped_and_unmapped_tensors_in_one_call(hp):
    a, ta, map_a, m_a, live_a, nan_a = mapped_pair(65, 200, "every-third", 60)
    c, tc, map_c, m_c, live_c, nan_c = mapped_pair(1000, 8, "stale", 61, t0=0)
    b, d = make_seg(1027, 62, True, 3), make_seg(3, 63, False, 0)
    tb, td = twin_of(b), twin_of(d)
    assert launch_multi(hp, [a, b, c, d], 1e-2, [(map_a, 200, STAMP), None, (map_c, 8, STAMP), None]) == 0, hp.lib.okge_last_error()
    step_in_pairs(hp, [ta, tb, tc, td], 1e-2)
    assert_same("mixed-mapped", [a, c], [ta, tc], cleared=False)
    assert_same("mixed-dense", [b, d], [tb, td])
    check_mapped("mixed-a", a, map_a, m_a, live_a, nan_a)
    check_mapped("mixed-c", c, map_c, m_c, live_c, nan_c)
