"""Sliding-window scene prediction without a GPU: the tile plan of iswm_scene_plan_make against the restatement
tests/scene_ref.py and its properties, the blend's own properties, the exported entry points and their host
validation, and the error caps of tests/test_scene_gpu.py checked on that test's inputs before a GPU sees them."""
import ctypes

import numpy as np
import pytest

from tests import predict_ref as R
from tests import scene_cases as SC
from tests import scene_ref as S


def _legal_overlaps(T):
    return range(0, T // 2 + 1)


def test_plan_matches_restatement_and_covers():
    from iswm_amd import ops
    checked = 0
    for T in range(2, 41):
        for L in range(1, 201):
            t = min(T, L)
            for O in _legal_overlaps(t) if L > t else (0, T // 2, T):
                t_, s, n, org = S.plan_axis(L, T, O)
                pl = ops.scene_plan(L, 1, T, O)                    # the axis under test is H; W = 1 is one window
                assert (pl.H, pl.th, pl.sy, pl.nty, pl.ramp) == (L, t_, s, n, max(O, 1)), (L, T, O)
                assert pl.origins_y() == org
                cover = np.zeros(L, dtype=int)
                for o in org:
                    assert 0 <= o <= L - t_
                    cover[o:o + t_] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (L, T, O)
                assert len(set(org)) == n and org == sorted(org)
                checked += 1
    assert checked > 50000
    # the other axis, and the scene the feature is for
    pl = ops.scene_plan(7, 53, 16, 4)
    assert pl.astuple() == S.Plan(7, 53, 16, 4).astuple() and pl.origins_x() == [0, 12, 24, 36, 37]
    pl = ops.scene_plan(6000, 6000, 513, 64)
    assert pl.astuple() == S.Plan(6000, 6000, 513, 64).astuple() and (pl.nty, pl.ntx, pl.ntiles) == (14, 14, 196)
    assert pl.origins_y()[-2:] == [12 * 449, 6000 - 513]


@pytest.mark.parametrize("lto,origins", [((37, 16, 4), [0, 12, 21]), ((53, 16, 4), [0, 12, 24, 36, 37]),
                                         ((129, 65, 16), [0, 49, 64]), ((33, 16, 0), [0, 16, 17])])
def test_plan_worked_examples(lto, origins):
    from iswm_amd import ops
    L, T, O = lto
    assert S.plan_axis(L, T, O)[3] == origins
    assert ops.scene_plan(L, L, T, O).origins_y() == origins == ops.scene_plan(L, L, T, O).origins_x()
    assert len(S.plan_axis(6000, 513, 64)[3]) == 14


def test_plan_errors_name_both_numbers():
    from iswm_amd import ops
    from iswm_amd._lib import IswmError
    with pytest.raises(IswmError, match=r"overlap 9 .*16"):
        ops.scene_plan(40, 40, 16, 9)                              # O > t / 2
    with pytest.raises(IswmError, match=r"overlap 9 .*16.*width 40"):
        ops.scene_plan(10, 40, 16, 9)                              # the short axis is one window; the long one refuses
    assert ops.scene_plan(10, 12, 16, 9).ntiles == 1               # one window per axis: any overlap <= 1024
    with pytest.raises(IswmError, match=r"overlap 1025 .*4096"):
        ops.scene_plan(9000, 9000, 4096, 1025)
    with pytest.raises(IswmError, match=r"tile 0"):
        ops.scene_plan(40, 40, 0, 0)
    with pytest.raises(IswmError, match=r"0 x 40"):
        ops.scene_plan(0, 40, 16, 4)
    with pytest.raises(IswmError, match=r"overlap -1"):
        ops.scene_plan(40, 40, 16, -1)
    for bad in ((40, 40, 16, 9), (0, 40, 16, 4), (40, 40, 0, 0), (40, 40, 16, 1025)):
        with pytest.raises(ValueError):
            S.Plan(*bad)


def test_blend_single_tile_is_the_identity():
    rng = np.random.default_rng(0)
    for H, W, T, O in ((33, 33, 513, 64), (7, 9, 9, 4), (1, 1, 16, 0)):
        pl = S.Plan(H, W, T, O)
        assert pl.nty * pl.ntx == 1
        p = rng.random((1, H, W))
        assert np.array_equal(S.blend(p, pl, np.float64), p[0])
        p32 = p.astype(np.float32)
        assert np.array_equal(S.blend(p32, pl, np.float32), p32[0])


@pytest.mark.parametrize("scene", SC.SCENES)
def test_blend_constant_and_mirror(scene):
    H, W, T, O, _ = scene
    pl = S.Plan(H, W, T, O)
    n = pl.nty * pl.ntx
    for c in (0.0, 0.3, 1.0):
        out = S.blend(np.full((n, pl.th, pl.tw), c), pl, np.float64)
        assert np.abs(out - c).max() <= 1e-15
    w, total = S.weights(pl)
    assert w.min() >= 1 and w.max() <= pl.ramp ** 2 and total.max() <= 9 * pl.ramp ** 2 < 2 ** 24
    # mirrored in x: origins W - tw - ox, windows renumbered, data flipped -> the flipped result (the weights are
    # exact integers; the fp64 sums run in the opposite order)
    rng = np.random.default_rng(H)
    p = rng.random((pl.nty, pl.ntx, pl.th, pl.tw))
    out = S.blend(p.reshape(n, pl.th, pl.tw), pl, np.float64)
    mp = S.Plan(H, W, T, O)
    mp.ox = sorted(W - pl.tw - o for o in pl.ox)
    out_m = S.blend(p[:, ::-1, :, ::-1].reshape(n, pl.th, pl.tw), mp, np.float64)
    assert np.abs(out_m - out[:, ::-1]).max() <= 4e-16


def _aligned(buf):
    a = ctypes.addressof(buf)
    return ctypes.c_void_p((a + 15) // 16 * 16)


def test_scene_entry_points_are_exported_and_validate_on_the_host():
    from iswm_amd import _lib, ops
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    for n in ("iswm_scene_plan_make", "iswm_scene_tiles_normalize", "iswm_scene_maps_workspace", "iswm_scene_maps"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert ctypes.sizeof(_lib.ScenePlan) == 36
    buf = (ctypes.c_char * 256)()
    p = _aligned(buf)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    pl = ops.scene_plan(37, 53, 16, 4)
    ref = ctypes.byref(pl)
    # workspace: one 32-byte partial per workgroup of predict_maps' grid for one image
    assert lib.iswm_scene_maps_workspace(37, 53) == lib.iswm_predict_maps_workspace(1, 37, 53) == 32
    assert lib.iswm_scene_maps_workspace(0, 53) == 0
    ws = lib.iswm_scene_maps_workspace(37, 53)
    assert lib.iswm_scene_plan_make(37, 53, 16, 4, None) == 1 and "null" in err()
    # null pointers, bad ranges, an inconsistent plan: status 1 and a message, nothing launched
    assert lib.iswm_scene_tiles_normalize(None, ref, 0, 1, f3, f3, p, None) == 1 and "null" in err()
    assert lib.iswm_scene_tiles_normalize(p, None, 0, 1, f3, f3, p, None) == 1 and "null" in err()
    assert lib.iswm_scene_tiles_normalize(p, ref, 14, 2, f3, f3, p, None) == 1 and "outside" in err()
    assert lib.iswm_scene_tiles_normalize(p, ref, -1, 1, f3, f3, p, None) == 1
    assert lib.iswm_scene_tiles_normalize(p, ref, 0, 0, f3, f3, p, None) == 1
    args = lambda yl=p, plan=ref, ldx=4, C=2, fg=1, out=p, wsb=ws: (yl, plan, 5, 5, ldx, C, fg, 0.5, 51, 178, out, p, p,
                                                                      None, p, p, wsb, None)
    assert lib.iswm_scene_maps(*args(yl=None)) == 1 and "null" in err()
    assert lib.iswm_scene_maps(*args(plan=None)) == 1 and "null" in err()
    assert lib.iswm_scene_maps(*args(wsb=ws - 1)) == 1 and "workspace" in err()
    assert lib.iswm_scene_maps(*args(fg=2)) == 1 and "foreground class 2" in err()
    assert lib.iswm_scene_maps(*args(ldx=6)) == 1 and "ldx" in err()
    assert lib.iswm_scene_maps(*args(C=5)) == 1 and "ldx" in err()
    assert lib.iswm_scene_maps(*args(out=ctypes.c_void_p(p.value + 4))) == 1 and "aligned" in err()
    for field, value in (("sy", 0), ("sy", 7), ("nty", 2), ("nty", 4), ("th", 38), ("ramp", 0), ("ramp", 1025), ("H", 0)):
        bad = _lib.ScenePlan(*pl.astuple())
        setattr(bad, field, value)
        assert lib.iswm_scene_maps(*args(plan=ctypes.byref(bad))) == 1 and "plan" in err(), (field, value)
        assert lib.iswm_scene_tiles_normalize(p, ctypes.byref(bad), 0, 1, f3, f3, p, None) == 1 and "plan" in err()


@pytest.mark.parametrize("scene", SC.SCENES)
@pytest.mark.parametrize("c,fg,ld", SC.CLASSES)
def test_blend_fp32_respects_the_gpu_tests_caps(c, fg, ld, scene):
    """the kernel's order of operations in float32 against the definition in float64, on the GPU test's logits with
    each window's probability correctly rounded: both caps of test_scene_maps_against_restatement hold"""
    H, W, T, O, side = scene
    pl = S.Plan(H, W, T, O)
    n = pl.nty * pl.ntx
    yl = SC.scene_logits(n, side, c, fg, ld).numpy()
    p_t = R.softmax_fg(SC.upsample64(yl, c, pl.th, pl.tw), fg)
    p64 = S.blend(p_t, pl, np.float64)
    p32 = S.blend(p_t.astype(np.float32), pl, np.float32)
    assert np.abs(p32.astype(np.float64) - p64).max() <= SC.BOUND
    for thr, mn, mx in SC.CUTS:
        pred, conf = R.predict_mask(p32, thr)
        band = R.binarize_confidence_map(conf, mn, mx)
        pred_r, conf_r = R.predict_mask(p64, thr)
        band_r = R.binarize_confidence_map(conf_r, mn, mx)
        bad = (pred != pred_r) | (conf != conf_r) | (band != band_r)
        edge = R.near_boundary(p64, thr, 2 * SC.BOUND)
        assert not (bad & ~edge).any()
        assert (bad & ~(p32 == 1.0)).sum() <= 1e-3 * p64.size + 2


def test_tile_flags_parse_and_refuse_bad_combinations(capsys):
    from iswm_amd import predict
    parser = predict.get_argparser()
    base = ["--input", "x", "--save_val_results_to", "y"]
    opt = lambda *a: predict.tile_options(parser, parser.parse_args(base + list(a)))
    assert opt() == (0, 0)                                          # absent: the whole-frame path
    assert opt("--tile_size", "513") == (513, 64)                   # default overlap: tile_size // 8
    assert opt("--tile_size", "513", "--tile_overlap", "0") == (513, 0)
    assert opt("--tile_size", "16", "--tile_overlap", "8") == (16, 8)
    for bad in (("--tile_overlap", "4"), ("--tile_size", "-1"), ("--tile_size", "16", "--tile_overlap", "9"),
                ("--tile_size", "16", "--tile_overlap", "-2"), ("--tile_size", "4096", "--tile_overlap", "1025")):
        with pytest.raises(SystemExit):
            opt(*bad)
        assert "--tile_" in capsys.readouterr().err
