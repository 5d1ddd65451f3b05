"""The ctypes binding is derived from include/iswm_hip.h (iswm_amd/_lib.py): the record layouts, one hand-written signature per
type form, the constants and the Python names that read them, what the parser refuses and accepts, and that importing the
binding loads neither torch nor the library.  No GPU, no library."""
import ctypes
import os
import subprocess
import sys
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

from iswm_amd import _lib

P = c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = {"ISWM_ACT_NONE": 0, "ISWM_ACT_RELU": 1, "ISWM_ACT_RELU6": 6, "ISWM_GATE_NONE": 0, "ISWM_GATE_RECOMPUTED": 2,
             "ISWM_GATE_RESIDUAL": 3, "ISWM_AUG_OP_BRIGHTNESS": 0, "ISWM_AUG_OP_CONTRAST": 1, "ISWM_AUG_OP_SATURATION": 2,
             "ISWM_AUG_OP_HUE": 3, "ISWM_PREDICT_MAX_VIEWS": 16}


def test_record_sizes_and_offsets():
    sizes = [(name, ctypes.sizeof(rec)) for name, rec in _lib.STRUCTS.items()]
    assert sizes == [("iswm_conv_desc", 56), ("iswm_pack_job", 40), ("iswm_aug_sample", 64), ("iswm_aug_extra", 96),
                     ("iswm_scene_plan", 36), ("iswm_predict_view", 24), ("iswm_qconv_desc", 76)]
    extra = _lib.STRUCTS["iswm_aug_extra"]
    assert (extra.rot_img_off.offset, extra.factor.offset, extra.hue_shift.offset) == (32, 64, 80)
    assert _lib.ConvDesc is _lib.STRUCTS["iswm_conv_desc"] and _lib.QConvDesc is _lib.STRUCTS["iswm_qconv_desc"]
    assert _lib.PredictView is _lib.STRUCTS["iswm_predict_view"]
    assert issubclass(_lib.ScenePlan, _lib.STRUCTS["iswm_scene_plan"])
    assert ctypes.sizeof(_lib.ScenePlan) == 36
    d = _lib.ConvDesc(16, 33, 35, 64, 17, 18, 128, 3, 3, 2, 1, 1, 64, 128)         # positional, in the header's order
    assert (d.N, d.W, d.Cout, d.stride, d.ldx, d.ldy) == (16, 35, 128, 2, 64, 128)
    plan = _lib.ScenePlan(100, 90, 64, 64, 48, 48, 2, 2, 16)
    assert plan.astuple() == (100, 90, 64, 64, 48, 48, 2, 2, 16) and plan.ntiles == 4
    assert plan.origins_y() == [0, 36] and plan.origins_x() == [0, 26]


SIGNATURES = {
    "iswm_last_error": (c_char_p, []),
    "iswm_lovasz_workspace": (c_int64, [c_int64, c_int64]),
    "iswm_dropout_fwd": (c_int, [P, P, P, c_int64, c_float, c_uint64, c_uint64, P]),
    "iswm_overlap_loss_coeffs": (c_int, [P, c_int, c_double, c_double, c_double, c_double, c_double, c_double, c_int, P, P, P]),
    "iswm_conv2d_kernel_name": (c_int, [POINTER(_lib.ConvDesc), c_int, c_char_p, c_int]),
    "iswm_aspp_fwd": (c_int, [POINTER(_lib.ConvDesc), c_int, P, P, P, P, c_int64, P, P, P, P]),
    "iswm_scene_plan_make": (c_int, [c_int, c_int, c_int, c_int, POINTER(_lib.STRUCTS["iswm_scene_plan"])]),
    "iswm_predict_views_maps": (c_int, [POINTER(_lib.PredictView), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                        c_int, c_int, P, P, P, P, P, P, c_size_t, P]),
    "iswm_pack_weights_batch": (c_int, [P, c_int, c_int, P]),
    "iswm_aug_rotate": (c_int, [P, P, P, P, c_int, c_int64, P, c_size_t, P, c_size_t, P]),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature(name):
    assert _lib._SIGS[name] == SIGNATURES[name]


def test_constants_and_their_python_names():
    from iswm_amd import ops
    from iswm_amd.utils import ext_transforms as et
    assert _lib.CONSTANTS == CONSTANTS
    assert {a.name: int(a) for a in ops.Act} == {"NONE": 0, "RELU": 1, "RELU6": 6}
    for a in ops.Act:
        assert int(a) == _lib.CONSTANTS["ISWM_ACT_" + a.name]
    for n in ("NONE", "RECOMPUTED", "RESIDUAL"):
        assert getattr(ops, "GATE_" + n) == _lib.CONSTANTS["ISWM_GATE_" + n]
    assert ops.PREDICT_MAX_VIEWS == _lib.CONSTANTS["ISWM_PREDICT_MAX_VIEWS"]
    for n in ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE"):
        assert getattr(et, "OP_" + n) == _lib.CONSTANTS["ISWM_AUG_OP_" + n]
    assert ctypes.sizeof(ctypes.c_longlong) == 8        # `long long` is bound as c_int64


def test_exports_are_the_prototypes_in_header_order():
    assert len(_lib.EXPORTS) == 162 == len(set(_lib.EXPORTS))
    assert _lib.EXPORTS[:2] == ("iswm_last_error", "iswm_version") and _lib.EXPORTS[-1] == "iswm_swap_f32"


@pytest.mark.parametrize("text,named", [
    ("int iswm_f(short a);", "int iswm_f(short a)"),                                    # a scalar outside the table
    ("int iswm_f(mystery_t* a);", "int iswm_f(mystery_t* a)"),                          # a pointee outside it
    ("int iswm_f(int n, int (*cb)(int));", "int iswm_f(int n, int (*cb)(int))"),        # a function pointer
    ("typedef struct { int a : 3; int b; } iswm_r;", "typedef struct { int a : 3; int b; } iswm_r"),      # a bit-field
    ("int iswm_f(int a;\nint iswm_g(void);", "int iswm_f(int a"),                       # unbalanced parentheses
    ("int iswm_f(int a))(;", "int iswm_f(int a))("),
    ("int iswm_f(int a)", "int iswm_f(int a)"),                                         # no `;`
    ("int iswm_f(int);", "int iswm_f(int)"),                                            # an unnamed parameter
    ("typedef struct { int a[]; } iswm_r;", "typedef struct { int a[]; } iswm_r"),
    ("typedef struct { int *a, b; } iswm_r;", "typedef struct { int *a, b; } iswm_r"),
    ("enum { ISWM_A = 1, ISWM_B };", "enum { ISWM_A = 1, ISWM_B }"),
    ("#define ISWM_N (1 << 4)\n", "#define ISWM_N (1 << 4)"),
])
def test_parser_refuses_what_it_does_not_know(text, named):
    with pytest.raises(ValueError) as e:
        _lib.parse_header(text)
    assert named in str(e.value)


def test_parser_accepts_the_forms_of_the_header():
    constants, structs, sigs = _lib.parse_header("""
        /* a comment with int bogus(short x); inside */
        #ifndef GUARD_H
        #define GUARD_H
        #include <stdint.h>
        #define ISWM_N 4   /* trailing comment */
        extern "C" {
        typedef void* iswm_stream_t; // hipStream_t
        enum { ISWM_A = 0, ISWM_B = 0x10 };
        typedef struct iswm_r { const float* w; int H, W; long long off; float f[ISWM_N_IS_NOT_EXPANDED]; } iswm_r;
        }
        #endif
    """.replace("ISWM_N_IS_NOT_EXPANDED", "4"))
    assert constants == {"ISWM_N": 4, "ISWM_A": 0, "ISWM_B": 16} and sigs == {}
    assert structs["iswm_r"]._fields_ == [("w", c_void_p), ("H", c_int), ("W", c_int), ("off", c_int64), ("f", c_float * 4)]
    _, structs, sigs = _lib.parse_header("""
        typedef void* iswm_stream_t;
        typedef struct { int a; } iswm_r;
        int iswm_f(const void* const* p, float* const* q, int k[], double** r, const iswm_r* d, iswm_r** dd,
                   const unsigned char* img, char* buf, uint8_t* idx, iswm_stream_t stream);
        const char* iswm_g(void);
        size_t
        iswm_h(
            int64_t n,
            uint64_t seed
        );
        long long iswm_i();
    """)
    assert sigs == {"iswm_f": (c_int, [P, P, P, P, POINTER(structs["iswm_r"]), P, P, c_char_p, P, P]),
                    "iswm_g": (c_char_p, []), "iswm_h": (c_size_t, [c_int64, c_uint64]), "iswm_i": (c_int64, [])}
    assert list(sigs) == ["iswm_f", "iswm_g", "iswm_h", "iswm_i"]


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys; import iswm_amd._lib as L; import iswm_amd.utils.ext_transforms; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert L._lib is None, 'the library was loaded'")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
