"""tests/dw3_pre_ref.py on the CPU (no GPU): the extension header and its binding, which layout and chunking every case of
tests/test_dwconv3_pre_gpu.py reaches, and the faults its assertions catch.

Emulated faults: each is applied to the float64 tap-level restatement of a case that reaches the branch and must miss an
assertion of the GPU file by >= 3 x the bound that assertion uses there (4 x the floor computed here as the GPU file computes it;
an equality assertion: differ at all, printed as inf).  A fault that is the same function on a case says so.  `pytest -s` prints
the table."""
import ctypes
import os
import re

import pytest
import torch

from iswm_amd import _lib
from tests import dw3_pre_ref as D
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSITIVITY = 3.0


# ---- the extension header ------------------------------------------------------------------------------------------------------
def test_extension_header_binds_into_a_table_of_its_own():
    text = open(os.path.join(ROOT, "include", "iswm_hip_sep.h")).read()
    constants, structs, sigs = _lib.parse_header(text, base=open(_lib.HEADER).read())
    assert constants == {} and structs == {}                                    # prototypes only: no record, no ISWM_ constant
    assert not re.search(r"^[ \t]*#[ \t]*define[ \t]+ISWM_\w+[ \t]+\S", text, re.M)       # (the include guard has no value)
    assert tuple(sigs) == _lib.EXT_EXPORTS == ("iswm_dwconv3x3_pre_fwd", "iswm_dwconv3x3_pre_bwd_workspace", "iswm_dwconv3x3_pre_bwd")
    assert set(re.findall(r"\b(iswm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))) == set(_lib.EXT_EXPORTS)
    assert not set(_lib.EXT_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 162
    P, desc = ctypes.c_void_p, ctypes.POINTER(_lib.ConvDesc)                    # the main header's record class, not a copy
    assert _lib._EXT_SIGS["iswm_dwconv3x3_pre_fwd"] == (ctypes.c_int, [desc, P, P, ctypes.c_int, ctypes.c_int, P, ctypes.c_int64,
                                                                      ctypes.c_int, P])
    assert _lib._EXT_SIGS["iswm_dwconv3x3_pre_bwd_workspace"] == (ctypes.c_size_t, [desc])
    assert _lib._EXT_SIGS["iswm_dwconv3x3_pre_bwd"][1][:2] == [desc, P] and len(_lib._EXT_SIGS["iswm_dwconv3x3_pre_bwd"][1]) == 13
    with pytest.raises(ValueError):                                             # a name of the main header declared again
        _lib.parse_header("int iswm_version(void);", base=open(_lib.HEADER).read())
    with pytest.raises(ValueError):                                             # the types of the main header need `base`
        _lib.parse_header(text)


def test_every_extension_entry_point_is_a_symbol_of_the_library():
    assert os.path.exists(_lib.LIB_PATH), "libiswm_hip.so is not built"
    lib = _lib.load()
    for name in _lib.EXT_EXPORTS:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == _lib._EXT_SIGS[name]


# ---- which branch every case reaches --------------------------------------------------------------------------------------------
def test_cases_cover_what_the_issue_of_the_models_needs():
    cases = D.CASES
    assert {(c[3], c[4]) for c in cases} >= {(64, 64), (128, 128), (728, 736), (728, 768), (1536, 1536), (20, 20)}
    assert {(c[7], c[8]) for c in cases} >= D.DIL_PAD_OS16 | D.DIL_PAD_OS8
    assert {c[9] for c in cases} == {True, False}
    assert any(c[:3] == (2, 13, 11) for c in cases) and any(c[:3] == (1, 1, 1) for c in cases)
    assert any(c[2] == 1 and c[1] > 1 for c in cases)                                        # one column
    assert any(c[1] <= c[7] and c[2] <= c[7] and c[1] * c[2] > 1 for c in cases)             # H, W <= dil
    small = [c for c in cases if c[:3] == (1, 7, 9)][0]
    assert small[7:9] == (4, 1) and D.out_hw(small) == (1, 3)
    assert D.out_hw((1, 6, 9, 128, 128, 128, 1, 4, 1, True))[0] == 0                          # one row fewer: no output
    assert len(set(D.case_id(c) for c in cases + D.BIG_BWD)) == len(cases + D.BIG_BWD)
    for c in cases:
        assert min(D.out_hw(c)) >= 1, c


def test_layouts():
    """the forward lays its quads over the pitch of y: 728 channels in 768 columns (the pitch the Xception pointwise convs read,
    12 x 64 for the planes kernels) are 12 full blocks of 16 quads, in 736 columns 23 blocks of 8; over 728 itself they would
    be the fallback.  20 channels are the fallback in both directions."""
    assert D.layout(736) == (8, 32, 23, False) and D.layout(728)[3] and D.layout(768) == (16, 16, 12, False)
    assert D.layout(64) == (16, 16, 1, False) and D.layout(128) == (16, 16, 2, False) and D.layout(1536) == (16, 16, 24, False)
    assert D.layout(20) == (16, 16, 1, True)
    assert D.bwd_layout(728) == (8, 32, 23, False) and D.bwd_layout(20) == D.layout(20) and D.bwd_layout(1536) == D.layout(1536)
    same = [c for c in D.CASES if c[7] == c[8] and D.bwd_layout(c[3]) == D.layout(c[3])]
    assert len(same) >= 5 and {c[9] for c in same} == {True, False}        # where dw is held to iswm_dwconv3x3_bwd bit for bit
    from iswm_amd.network.backbone.xception import PointwiseConv2d
    assert PointwiseConv2d(728, 728, 1, bias=False).cin_p == 768 and PointwiseConv2d(64, 128, 1, bias=False).cin_p == 64


def test_backward_chunking():
    for case in D.CASES:
        q = D.queries(case)
        assert q["chunks"] == min(2048, max(1, (q["pout"] + 255) // 256)) and q["out_chunk"] <= 256, case
    assert max(D.queries(c)["chunks"] for c in D.CASES) >= 2                                  # more than one workgroup partial
    q = D.queries(D.BIG_BWD[0])
    assert q["chunks"] == 2048 and q["pout"] > 2048 * 256 and q["out_chunk"] == 257 == q["in_chunk"] and q["pout"] % 257 == 60
    # pad < dil: the input grid is larger than the output grid, so the two chunk sizes differ
    q = D.queries(D.CASES[1])
    assert q["pin"] == 2 * 13 * 11 and q["pout"] == 2 * 11 * 9 and q["in_chunk"] > q["out_chunk"]
    # a map with no output has no workspace (and the entry points refuse it)
    d = _lib.ConvDesc(1, 3, 3, 8, 0, 0, 8, 3, 3, 1, 1, 4, 8, 8)
    assert _lib.load().iswm_dwconv3x3_pre_bwd_workspace(ctypes.byref(d)) == 0


# ---- the tap-level restatement is the float64 operator ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=[D.case_id(c) for c in D.CASES])
def test_restatement_is_the_tap_formula(case):
    r = D.inputs(case)
    ref, cw = D.restate(case, r), case[5]
    assert rel_err(D.y_by_taps(case, r), ref["y"][..., :cw]) < 1e-14
    assert rel_err(D.dx_by_taps(case, r), ref["dx"][..., :cw]) < 1e-14
    assert rel_err(D.dw_by_chunks(case, r, D.queries(case)["out_chunk"]), ref["dw"]) < 1e-13
    if case[9]:
        x = r["x"]
        assert int((x == 0).sum()) > 0 and bool(torch.signbit(x[x == 0]).any()) and bool((~torch.signbit(x[x == 0])).any())
        assert float(ref["dx"][..., :cw][x[..., :cw] <= 0].abs().max()) == 0.0                 # torch's convention: 0 at x <= 0


# ---- faults ----------------------------------------------------------------------------------------------------------------------
def row(fault, case, what, ratio):
    print("fault %-58s %-42s %-10s %s" % (fault, D.case_id(case), what, "same function on this case" if ratio is None else "%.3g x bound" % ratio))
    assert ratio is None or ratio >= SENSITIVITY, (fault, D.case_id(case), what, ratio)


def _ctx(case, ch=None):
    r = D.inputs(case)
    ref = D.restate(case, r, ch)
    return r, ref, {k: 4.0 * v for k, v in D.floors(case, r, ref, ch).items()}


def test_fault_mask_from_the_rectified_value():
    """mask = relu(x) > 0 selects the same elements as x > 0 (shown); what a wrong comparison on the un-rectified x lets through
    is x == 0: `x >= 0` passes the planted +0.0 / -0.0, which `dx == 0 where x <= 0` catches"""
    case = D.CASES[0]
    r, ref, b = _ctx(case)
    good = D.dx_by_taps(case, r)
    row("mask taken from relu(x) > 0 instead of x > 0", case, "dx", None if torch.equal(D.dx_by_taps(case, r, "relu(x)>0"), good) else 0.0)
    mut = D.dx_by_taps(case, r, "x>=0")
    leaked = float(mut[r["x"] <= 0].abs().max())
    row("mask taken as x >= 0 (or from relu(x) >= 0)", case, "dx==0", float("inf") if leaked > 0 else 0.0)
    row("... against float64", case, "dx", rel_err(mut, ref["dx"]) / b["dx"])


def test_fault_mask_on_the_weight_gradient_operand_only():
    for case in (D.CASES[0], D.CASES[2]):
        r, ref, b = _ctx(case)
        cw = case[5]
        mut = D.dx_by_taps(case, r, "none")
        row("relu on dw's operand, dx left unmasked", case, "dx", rel_err(mut, ref["dx"][..., :cw]) / b["dx"])
        row("... the converse: dx masked, dw from the un-rectified x", case, "dw",
            rel_err(D.dw_by_chunks(case, r, D.queries(case)["out_chunk"], relu_of=False), ref["dw"]) / b["dw"])


def test_fault_pad_taken_as_dil():
    for case in [c for c in D.CASES if c[8] < c[7]]:
        r, ref, b = _ctx(case)
        cw = case[5]
        row("taps at -dil + k dil (pad taken as dil)", case, "y", rel_err(D.y_by_taps(case, r, pad=case[7]), ref["y"][..., :cw]) / b["y"])
        row("... in the data gradient", case, "dx", rel_err(D.dx_by_taps(case, r, pad=case[7]), ref["dx"][..., :cw]) / b["dx"])
    assert len([c for c in D.CASES if c[8] < c[7]]) >= 5


def test_fault_chunk_drops_its_last_pixel():
    """on the shape under the chunk cap (257-pixel chunks) and on a small case with several chunks"""
    big = D.BIG_BWD[0]
    two = [c for c in D.CASES if c[:3] == (2, 17, 15)][0]
    for case, ch in ((two, None), (big, D.subset_channels(big[3], big[5])[:4])):
        r, ref, b = _ctx(case, ch)
        q = D.queries(case)
        if ch is not None:                                 # the tap model runs on the channel subset
            r = dict(r, x=r["x"][..., ch], dy=r["dy"][..., ch], w=r["w"][ch], dx0=r["dx0"][..., ch])
            case_m = case[:3] + (len(ch), len(ch), len(ch)) + case[6:]
        else:
            case_m = case
        assert q["chunks"] >= 2 and case[8] == 1 and (case is big or q["in_chunk"] > q["out_chunk"])
        mut = D.dw_by_chunks(case_m, r, q["out_chunk"], drop_last=True)
        row("a chunk drops its last output pixel (out_chunk %d)" % q["out_chunk"], case, "dw", rel_err(mut, ref["dw"]) / b["dw"])
        mut = D.dx_by_taps(case_m, r, drop_last_of_chunk=q["in_chunk"])
        row("a chunk drops its last input pixel (in_chunk %d)" % q["in_chunk"], case, "dx", rel_err(mut, ref["dx"][..., :case_m[5]]) / b["dx"])


def test_fault_unzeroed_pad_columns():
    """the GPU file fills the output buffers with 7.0 / 1.0 before the call and asserts columns [C, pitch) == 0: a kernel that
    leaves them alone fails by the fill value; every case with pitch > C shows it"""
    wide = [c for c in D.CASES if c[4] > c[3]]
    assert len(wide) >= 2 and {c[9] for c in wide} == {True, False}
    for case in wide:
        row("columns [C, pitch) of y left unwritten", case, "pad==0", float("inf"))
