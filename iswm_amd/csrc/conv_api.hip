// Host side of the convolution C ABI: the conv-math state, the route planner and the entry points of every kernel family
// (fp32 conv_mfma.hip, tap-uniform conv_mfma_u.hip, bf16x6 conv_mfma_x6*.hip, planes conv_mfma_pl2*.hip, conv_stem.hip).
// No kernel lives here.
//
// A route is decided ONCE: plan_route() (forward / data gradient) and plan_wgrad() / plan_wgrad_pl() (weight gradients) turn
// (descriptor, entry point, conv math) into the kernel family, its template parameters and the BatchNorm-partial layout.
// The entry points launch what the plan says; iswm_conv2d_kernel_name and the layout / workspace queries format the same
// plan.  The conv math is read once per C call and passed down.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "conv_common.h"

using namespace iswm;

// 0: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32);  1 (default): bf16x6 split on the bf16 matrix cores;  2: bf16.
// -1 until the first read, which takes ISWM_CONV_MATH unless iswm_set_conv_math got there first.
static std::atomic<int> g_conv_math{-1};
static int conv_math() {
    int m = g_conv_math.load();
    if (m < 0) {
        const char* e = getenv("ISWM_CONV_MATH");
        const int env = (e && (!strcmp(e, "f32") || !strcmp(e, "0"))) ? 0
                        : (e && (!strcmp(e, "bf16") || !strcmp(e, "2"))) ? 2 : 1;   // default: bf16x6
        int unset = -1;
        g_conv_math.compare_exchange_strong(unset, env);      // a mode stored meanwhile by another thread stands
        m = g_conv_math.load();
    }
    return m;
}
extern "C" int iswm_set_conv_math(int mode) {
    ISWM_REQUIRE(mode >= 0 && mode <= 2, "set_conv_math: mode must be 0 (f32), 1 (bf16x6) or 2 (bf16)");
    g_conv_math = mode;
    return 0;
}
extern "C" int iswm_get_conv_math(void) { return conv_math(); }

static int validate(const iswm_conv_desc* d) {
    ISWM_REQUIRE(d != nullptr, "conv: null descriptor");
    ISWM_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "conv: empty tensor");
    ISWM_REQUIRE(d->Cin % 4 == 0 && d->Cout % 4 == 0, "conv: Cin (%d) and Cout (%d) must be multiples of 4",
                 d->Cin, d->Cout);
    ISWM_REQUIRE(d->ldx % 4 == 0 && d->ldy % 4 == 0 && d->ldx >= d->Cin && d->ldy >= d->Cout,
                 "conv: bad pixel pitch ldx=%d ldy=%d", d->ldx, d->ldy);
    ISWM_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->dil > 0 && d->pad >= 0, "conv: bad geometry");
    int ho = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
    int wo = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
    ISWM_REQUIRE(ho == d->Ho && wo == d->Wo, "conv: output size %dx%d does not match geometry (%dx%d)", d->Ho,
                 d->Wo, ho, wo);
    ISWM_REQUIRE((int64_t)d->N * d->H * d->W * d->ldx < (1ll << 31) &&
                     (int64_t)d->N * d->Ho * d->Wo * d->ldy < (1ll << 31),
                 "conv: tensor exceeds 2^31 elements");
    return 0;
}

// ConvArgs of a forward call; dgrad: of a data gradient -- a.x is the gathered operand (dy, pitch ldy), a.y the output (dx,
// pitch ldx), a.M / a.Ktot the data gradient's GEMM
static ConvArgs base_args(const iswm_conv_desc* d, bool dgrad = false) {
    ConvArgs a{};
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin;
    a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
    a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
    a.ldx = dgrad ? d->ldy : d->ldx; a.ldy = dgrad ? d->ldx : d->ldy;
    a.M = dgrad ? d->N * d->H * d->W : d->N * d->Ho * d->Wo;
    a.Ktot = d->KH * d->KW * (dgrad ? d->Cout : d->Cin);
    return a;
}

static PatchArgs patch_args(const iswm_conv_desc* d, bool dgrad, int PH, int PW) {
    PatchArgs p{};
    p.N = d->N;
    p.KH = d->KH; p.KW = d->KW; p.dil = d->dil;
    p.PH = PH; p.PW = PW;
    if (!dgrad) {
        p.RH = d->Ho; p.RW = d->Wo; p.GH = d->H; p.GW = d->W; p.GC = d->Cin; p.NC = d->Cout;
        p.orgh = -d->pad; p.orgw = -d->pad; p.flip = 0; p.ldg = d->ldx; p.ldo = d->ldy;
    } else {
        p.RH = d->H; p.RW = d->W; p.GH = d->Ho; p.GW = d->Wo; p.GC = d->Cout; p.NC = d->Cin;
        p.orgh = d->pad - d->dil * (d->KH - 1); p.orgw = d->pad - d->dil * (d->KW - 1);
        p.flip = 1; p.ldg = d->ldy; p.ldo = d->ldx;
    }
    return p;
}

// ---- The route of a forward / data-gradient call ----
enum ConvFamily { F_FP32, F_U, F_X6, F_X6_PK, F_X6_PATCH, F_PL2, F_PL2W, F_STEM };
enum ConvEntry { E_FWD, E_DGRAD, E_DGRAD_WT, E_FWD_PACKED, E_DGRAD_PACKED, E_FWD_PL2, E_DGRAD_PL2 };

struct ConvRoute {
    ConvFamily family;
    bool dgrad;
    int planes;             // bf16 planes per operand of the packed / planes kernels: 3 (bf16x6) or 1 (bf16)
    int bm, bn;             // F_FP32 (bm 128), F_U, F_X6, F_X6_PK (bn 64): tile
    int rbw, wm;            // F_PL2 / F_PL2W: 16-row blocks per tile; wave rows (2: the 64-column layout <rbw / 2, 2>)
    int PH, PW;             // F_X6_PATCH: patch
    int tiles, tile_rows;   // forward: rows of the BatchNorm partials and GEMM rows per tile (0: image patches, row counts stored)
    int stat_tiles;         // E_DGRAD_PL2: first dimension of the fused BatchNorm-backward statistics
};

// Tile-width choice of the fp32 kernels.  A CU works through ceil(tiles/256) tiles (co-resident workgroups share its SIMDs),
// so a 128x128 grid of 274 tiles (the 33x33 stages with 256 output channels) costs two full tile times where 128x64 tiles
// cost three half tile times.  Narrow tiles re-read the activation panel once more and pay ~10 % in MFMA:staging ratio.
static bool use_narrow_tile(int64_t MT, int cols) {
    if (cols <= 64 || (cols % 128 != 0 && cols % 128 <= 64)) return true;
    const int64_t t128 = MT * ((cols + 127) / 128), t64 = MT * ((cols + 63) / 64);
    const double c128 = (double)((t128 + 255) / 256) * 128.0;
    const double c64 = (double)((t64 + 255) / 256) * 64.0 * 1.10;
    return c64 < c128;
}

// e's own preconditions (validate; gathered channels % 32 for E_DGRAD_WT and the packed entries, % 64 for the planes entries)
// are the caller's
static ConvRoute plan_route(const iswm_conv_desc* d, ConvEntry e, int math) {
    ConvRoute r{};
    r.dgrad = e == E_DGRAD || e == E_DGRAD_WT || e == E_DGRAD_PACKED || e == E_DGRAD_PL2;
    r.planes = math_planes(math);
    const int64_t M = r.dgrad ? (int64_t)d->N * d->H * d->W : (int64_t)d->N * d->Ho * d->Wo;     // GEMM rows
    const int cols = r.dgrad ? d->Cin : d->Cout, gc = r.dgrad ? d->Cout : d->Cin;                // output columns, gathered channels
    const int taps = d->KH * d->KW, K = taps * gc;
    r.tile_rows = r.bm = 128;
    switch (e) {
    case E_FWD: case E_DGRAD: case E_DGRAD_WT:
        if (e == E_FWD && math == 1 && stem_geometry(base_args(d))) {
            r.family = F_STEM;
            r.tile_rows = stem_tile_rows();
        } else if (e == E_DGRAD_WT || (e == E_FWD && math == 1 && gc % 32 == 0)) {
            r.family = F_X6;                      // the plain data gradient never splits: its weights are not transposed
            conv_pick_tile_x6(M, cols, K, r.dgrad, taps == 1, &r.bm, &r.bn);
            r.tile_rows = r.bm;
        } else if (gc % 32 == 0) {
            r.family = F_U;
            conv_pick_tile(M, cols, &r.bm, &r.bn);
            r.tile_rows = r.bm;
        } else {
            r.family = F_FP32;
            r.bn = use_narrow_tile((M + 127) / 128, cols) ? 64 : 128;
        }
        break;
    case E_FWD_PACKED: case E_DGRAD_PACKED: {
        // halo patches: stride-1 K x K whose pixel grid fills 128-row patches well enough
        const int RH = r.dgrad ? d->H : d->Ho, RW = r.dgrad ? d->W : d->Wo;       // pixel grid of the GEMM rows
        if (d->stride == 1 && taps > 1 && conv_patch_plan(RH, RW, d->KH, d->KW, d->dil, &r.PH, &r.PW)) {
            r.family = F_X6_PATCH;
            r.tile_rows = 0;
            r.tiles = d->N * ((RH + r.PH - 1) / r.PH) * ((RW + r.PW - 1) / r.PW);
        } else {
            r.family = F_X6_PK;
            conv_pick_tile_x6(M, cols, K, r.dgrad, taps == 1, &r.bm, &r.bn);
            r.bn = 64;                            // the packed kernels have 64-column tiles only
            r.tile_rows = r.bm;
        }
        break;
    }
    case E_FWD_PL2: case E_DGRAD_PL2: {
        // the 256-column kernel (conv_mfma_pl2w.hip) is bf16x6 only; strided data gradients keep the parity-ordered rows of
        // k_conv_pl2, and a data gradient needs 8 stages per tile to pay
        const bool wide_ok = r.planes == 3 && (!r.dgrad || (d->stride == 1 && K >= 512));
        int wide;
        conv_pl2_plan(M, cols, K, wide_ok, &r.rbw, &wide, &r.wm);
        r.family = wide ? F_PL2W : F_PL2;
        r.tile_rows = 16 * r.rbw;
        break;
    }
    }
    if (r.tile_rows) r.tiles = (int)((M + r.tile_rows - 1) / r.tile_rows);
    r.stat_tiles = r.tiles * r.wm;                // narrow tiles: (rbw / 2) blocks x 2 wave rows, statistics per wave row
    return r;
}

static int route_name(const ConvRoute& r, char* buf, int buflen) {
    const char* dg = r.dgrad ? "true" : "false";
    switch (r.family) {
    case F_FP32: snprintf(buf, buflen, r.dgrad ? "k_conv_dgrad<%d>" : "k_conv_fwd<%d>", r.bn); break;
    case F_U: snprintf(buf, buflen, r.dgrad ? "k_conv_dgrad_u<%d, %d>" : "k_conv_fwd_u<%d, %d>", r.bm, r.bn); break;
    case F_X6: snprintf(buf, buflen, "k_conv_x6<%d, %d, %s, false, 3>", r.bm, r.bn, dg); break;
    case F_X6_PK: snprintf(buf, buflen, "k_conv_x6<%d, %d, %s, true, %d>", r.bm, r.bn, dg, r.planes); break;
    case F_X6_PATCH: snprintf(buf, buflen, "k_conv_x6_patch<%s, %d>", dg, r.planes); break;
    case F_PL2: snprintf(buf, buflen, "k_conv_pl2<%d, %d, %d, %s>", r.rbw / r.wm, r.wm, r.planes, dg); break;
    case F_PL2W: snprintf(buf, buflen, "k_conv_pl2w<%d, %d, %s>", r.rbw, r.planes, dg); break;
    case F_STEM: snprintf(buf, buflen, "k_stem_fwd<%d>", r.tile_rows / 16); break;
    }
    return 0;
}

// ---- The plan of iswm_conv2d_wgrad (fp32 operands): the stem's own kernel or k_conv_wgrad with its tile, pixel map and splits ----
static WgPlan plan_wgrad(const iswm_conv_desc* d, int math) {
    WgPlan p{};
    p.planes = math_planes(math);
    p.x6 = math >= 1;
    if (math == 1 && stem_geometry(base_args(d))) {
        p.kernel = 1;
        p.workspace = stem_wgrad_workspace(base_args(d));
        return p;
    }
    const int Ktot = d->KH * d->KW * d->Cin;
    p.bm = (d->Cout % 128 == 0) ? 128 : 64;
    p.bn = (p.bm == 128 && (Ktot % 128 == 0 || Ktot >= 1024)) ? 128 : 64;
    if (p.bn == 64) p.bm = 64;  // instantiated shapes: 128x128 and 64x64
    p.MT = (d->Cout + p.bm - 1) / p.bm;
    p.NT = (Ktot + p.bn - 1) / p.bn;
    const bool same = d->stride == 1 && d->Ho == d->H && d->Wo == d->W;
    p.mode = (same && d->KH == 1 && d->KW == 1 && d->pad == 0) ? 2 : (same ? 1 : 0);
    const int64_t P = (int64_t)d->N * d->Ho * d->Wo;
    const int64_t tiles = (int64_t)p.MT * p.NT;
    // Split count: minimise  rounds x (chunks per workgroup) x chunk time  +  slab write/read time, where a
    // round is 512 co-resident workgroups (2 per CU) and a 128x128x32 chunk takes ~4.5 us when two
    // workgroups share a CU.  tiles*splits just above a multiple of 512 costs a whole extra round.
    // (Three bf16x6 workgroups per CU fit in LDS and registers but measured no faster than two: r01 notes.)
    const int64_t slots = 512;
    const double chunk_us = 4.5 * (double)(p.bm * p.bn) / 16384.0;
    const double slab_us = (double)d->Cout * Ktot * 8.0 / 4.0e6;   // one slab written + read at ~4 TB/s
    int64_t maxs = (P + 255) / 256;                                 // at least 256 pixels per split
    if (maxs > 64) maxs = 64;
    double best = 1e300;
    p.psplit = (int)((P + 31) / 32 * 32);
    p.nsplit = 1;
    for (int64_t ns = 1; ns <= maxs; ++ns) {
        int64_t ps = ((P + ns - 1) / ns + 31) / 32 * 32;
        int64_t nsp = (P + ps - 1) / ps;
        int64_t rounds = (tiles * nsp + slots - 1) / slots;
        double t = (double)rounds * (double)(ps / 32 + 3) * chunk_us + (nsp > 1 ? (double)nsp * slab_us + 5.0 : 0.0);
        if (t < best) {
            best = t;
            p.psplit = (int)ps;
            p.nsplit = (int)nsp;
        }
    }
    if (p.nsplit > 1) p.workspace = (size_t)p.nsplit * d->Cout * Ktot * sizeof(float);
    return p;
}

// ---- Queries: plan, then format ----
/* 1 when iswm_conv2d_dgrad_wt (bf16x6 data gradient on transposed weights) applies to this geometry under
 * the current conv math */
static int dgrad_wants_wt(const iswm_conv_desc* d, int math) { return (d && math == 1 && d->Cout % 32 == 0) ? 1 : 0; }
extern "C" int iswm_conv2d_dgrad_wants_wt(const iswm_conv_desc* d) { return dgrad_wants_wt(d, conv_math()); }

extern "C" int iswm_conv2d_kernel_name(const iswm_conv_desc* d, int kind, char* buf, int buflen) {
    ISWM_REQUIRE(d && buf && buflen > 0 && kind >= 0 && kind <= 7, "kernel_name: bad argument");
    const int math = conv_math();
    if (kind == 7) {   // iswm_conv2d_wgrad_planes
        const WgPlan p = plan_wgrad_pl(d, math);
        snprintf(buf, buflen, p.kernel == 2 ? "k_wgrad_pls<%d>" : p.kernel == 1 ? "k_wgrad_plw<%d>" : "k_wgrad_pl<%d>", p.planes);
        return 0;
    }
    if (kind == 2) {   // iswm_conv2d_wgrad
        const WgPlan p = plan_wgrad(d, math);
        if (p.kernel == 1) snprintf(buf, buflen, "k_stem_wgrad");
        else snprintf(buf, buflen, "k_conv_wgrad<%d, %d, %d, %s, %d>", p.bm, p.bn, p.mode, p.x6 ? "true" : "false", p.planes);
        return 0;
    }
    // kind 1 names the data gradient the op wrappers call: iswm_conv2d_dgrad_wt where iswm_conv2d_dgrad_wants_wt says so,
    // else iswm_conv2d_dgrad
    static const ConvEntry entry[7] = {E_FWD, E_DGRAD, E_FWD, E_FWD_PACKED, E_DGRAD_PACKED, E_FWD_PL2, E_DGRAD_PL2};
    return route_name(plan_route(d, kind == 1 && dgrad_wants_wt(d, math) ? E_DGRAD_WT : entry[kind], math), buf, buflen);
}

extern "C" int iswm_conv2d_stat_tile_rows(const iswm_conv_desc* d) {
    return d ? plan_route(d, E_FWD, conv_math()).tile_rows : 0;
}

extern "C" int iswm_conv2d_stat_tiles(const iswm_conv_desc* d) {
    return d ? plan_route(d, E_FWD, conv_math()).tiles : 0;
}

/* BN-partials layout of iswm_conv2d_fwd_packed: *tile_rows == 0 means the tiles are image patches with varying
 * row counts, stored as floats after the two planes (partials + 2*tiles*Cout). */
extern "C" int iswm_conv2d_fwd_packed_stat_layout(const iswm_conv_desc* d, int* tiles, int* tile_rows) {
    ISWM_REQUIRE(d && tiles && tile_rows, "fwd_packed_stat_layout: null pointer");
    const ConvRoute r = plan_route(d, E_FWD_PACKED, conv_math());
    *tiles = r.tiles;
    *tile_rows = r.tile_rows;
    return 0;
}

/* tile rows of the planes kernels (conv_mfma_pl2*.hip): kind 0 forward (rows per BN partial), 1 data gradient */
extern "C" int iswm_conv2d_pl2_tile_rows(const iswm_conv_desc* d, int kind) {
    return d ? plan_route(d, kind ? E_DGRAD_PL2 : E_FWD_PL2, conv_math()).tile_rows : 0;
}

/* tile rows of the planes data gradient = first dimension of the statistics it can emit for the consumer BatchNorm backward */
extern "C" int iswm_conv2d_dgrad_pl2_stat_tiles(const iswm_conv_desc* d) {
    return (d && d->Cin > 0) ? plan_route(d, E_DGRAD_PL2, conv_math()).stat_tiles : 0;
}

extern "C" size_t iswm_conv2d_wgrad_workspace(const iswm_conv_desc* d) {
    return d ? plan_wgrad(d, conv_math()).workspace : 0;
}

// ---- fp32 operands, plain weights ----
extern "C" int iswm_conv2d_fwd(const iswm_conv_desc* d, const float* x, const float* w, const float* bias,
                               float* y, float* stat_partials, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(x && w && y, "conv_fwd: null pointer");
    ISWM_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "conv_fwd: pointers must be 16-byte aligned");
    ConvArgs a = base_args(d);
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.stats = stat_partials;
    hipStream_t s = (hipStream_t)stream;
    const ConvRoute r = plan_route(d, E_FWD, conv_math());
    switch (r.family) {
    case F_STEM:
        ISWM_REQUIRE(launch_stem_fwd(a, s), "conv_fwd: the stem kernel does not cover this geometry");
        return check_launch("stem_fwd");
    case F_X6:
        ISWM_REQUIRE(launch_conv_fwd_x6(a, s, r.bm, r.bn), "conv_fwd: no bf16x6 kernel for tile %d x %d", r.bm, r.bn);
        return check_launch("conv_fwd_x6");
    case F_U:
        ISWM_REQUIRE(launch_conv_fwd_u(a, s, r.bm, r.bn), "conv_fwd: no tap-uniform kernel for tile %d x %d", r.bm, r.bn);
        return check_launch("conv_fwd_u");
    default:
        launch_conv_fwd_f32(a, s, r.bn);
        return check_launch("conv_fwd");
    }
}

extern "C" int iswm_conv2d_dgrad(const iswm_conv_desc* d, const float* dy, const float* w, float* dx,
                                 int accumulate, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(dy && w && dx, "conv_dgrad: null pointer");
    ISWM_REQUIRE(aligned16(dy) && aligned16(w) && aligned16(dx), "conv_dgrad: pointers must be 16-byte aligned");
    ConvArgs a = base_args(d, true);
    a.x = dy; a.w = w; a.y = dx; a.accumulate = accumulate;
    hipStream_t s = (hipStream_t)stream;
    const ConvRoute r = plan_route(d, E_DGRAD, conv_math());
    if (r.family == F_U) {
        ISWM_REQUIRE(launch_conv_dgrad_u(a, s, r.bm, r.bn), "conv_dgrad: no tap-uniform kernel for tile %d x %d", r.bm, r.bn);
        return check_launch("conv_dgrad_u");
    }
    launch_conv_dgrad_f32(a, s, r.bn);
    return check_launch("conv_dgrad");
}

extern "C" int iswm_transpose_weights(const iswm_conv_desc* d, const float* w, float* wt, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(w && wt && w != wt, "transpose_weights: bad pointer");
    launch_transpose_ohwi(w, wt, d->Cout, d->KH * d->KW, d->Cin, (hipStream_t)stream);
    return check_launch("transpose_weights");
}

extern "C" int iswm_conv2d_dgrad_wt(const iswm_conv_desc* d, const float* dy, const float* wt, float* dx,
                                    int accumulate, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(dy && wt && dx, "conv_dgrad_wt: null pointer");
    ISWM_REQUIRE(aligned16(dy) && aligned16(wt) && aligned16(dx), "conv_dgrad_wt: pointers must be 16-byte aligned");
    ISWM_REQUIRE(d->Cout % 32 == 0, "conv_dgrad_wt: Cout must be a multiple of 32");
    ConvArgs a = base_args(d, true);
    a.x = dy; a.w = wt; a.y = dx; a.accumulate = accumulate;
    const ConvRoute r = plan_route(d, E_DGRAD_WT, conv_math());
    ISWM_REQUIRE(launch_conv_dgrad_x6(a, (hipStream_t)stream, r.bm, r.bn), "conv_dgrad_wt: no bf16x6 kernel for tile %d x %d",
                 r.bm, r.bn);
    return check_launch("conv_dgrad_x6");
}

extern "C" int iswm_conv2d_wgrad(const iswm_conv_desc* d, const float* x, const float* dy, float* dw,
                                 float* workspace, size_t workspace_bytes, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(x && dy && dw, "conv_wgrad: null pointer");
    ISWM_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dw), "conv_wgrad: pointers must be 16-byte aligned");
    const WgPlan p = plan_wgrad(d, conv_math());
    ISWM_REQUIRE(workspace_bytes >= p.workspace && (p.workspace == 0 || (workspace && aligned16(workspace))),
                 "conv_wgrad: workspace too small (%zu < %zu)", workspace_bytes, p.workspace);
    ConvArgs a = base_args(d);
    a.x = x; a.y = const_cast<float*>(dy);
    hipStream_t s = (hipStream_t)stream;
    if (p.kernel == 1) {
        ISWM_REQUIRE(launch_stem_wgrad(a, dw, workspace, s), "conv_wgrad: the stem kernel does not cover this geometry");
        return check_launch("stem_wgrad");
    }
    a.stats = (p.nsplit > 1) ? workspace : dw;
    launch_conv_wgrad(a, s, p);
    if (int e = check_launch("conv_wgrad")) return e;
    if (p.nsplit > 1) {
        launch_reduce_slabs(workspace, dw, (int64_t)d->Cout * a.Ktot / 4, p.nsplit, s);
        return check_launch("conv_wgrad_reduce");
    }
    return 0;
}

// ---- bf16x6 with pre-split, fragment-ordered weights ("packed"): kind 0 = forward, 1 = data gradient ----
extern "C" size_t iswm_conv2d_packed_weight_bytes(const iswm_conv_desc* d, int kind) {
    const int math = conv_math();
    if (!d || math < 1 || (kind != 0 && kind != 1)) return 0;
    const int gc = kind ? d->Cout : d->Cin;
    if (gc % 32 != 0) return 0;
    return packed_weight_bytes_x6(d->Cout, d->KH * d->KW, d->Cin, kind == 1, math_planes(math));
}

extern "C" int iswm_conv2d_pack_weights(const iswm_conv_desc* d, int kind, const float* w, void* packed,
                                        iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(kind == 0 || kind == 1, "pack_weights: kind must be 0 (forward) or 1 (data gradient)");
    ISWM_REQUIRE(w && packed && aligned16(packed), "pack_weights: bad pointer");
    ISWM_REQUIRE((kind ? d->Cout : d->Cin) % 32 == 0, "pack_weights: gathered channel count must be a multiple of 32");
    launch_pack_weights_x6(w, packed, d->Cout, d->KH * d->KW, d->Cin, kind == 1, math_planes(conv_math()), (hipStream_t)stream);
    return check_launch("pack_weights");
}

/* ---- batched packing: every conv of a model in one launch ---- */
static size_t packed_bytes(int Cout, int taps, int Cin, int kind, int math) {
    if (Cout <= 0 || taps <= 0 || Cin <= 0 || kind < 0 || kind > 3 || math < 1) return 0;
    if (kind >= 2) {        // planes kernels: gathered channel count a multiple of 64
        if (((kind == 3) ? Cout : Cin) % 64 != 0) return 0;
        return packed_weight_bytes_pl2(Cout, taps, Cin, kind == 3, math_planes(math));
    }
    if ((kind ? Cout : Cin) % 32 != 0) return 0;
    return packed_weight_bytes_x6(Cout, taps, Cin, kind == 1, math_planes(math));
}

extern "C" size_t iswm_packed_weight_bytes(int Cout, int taps, int Cin, int kind) {
    return packed_bytes(Cout, taps, Cin, kind, conv_math());
}

extern "C" int iswm_pack_job_blocks(int Cout, int taps, int Cin, int kind) {
    if (packed_bytes(Cout, taps, Cin, kind, conv_math()) == 0) return 0;
    if (kind >= 2) return pack_job_blocks_pl2(Cout, taps, Cin, kind == 3);
    return pack_job_blocks_x6(Cout, taps, Cin, kind == 1);
}

extern "C" int iswm_pack_weights_batch(const void* jobs_dev, int njobs, int total_blocks, iswm_stream_t stream) {
    ISWM_REQUIRE(jobs_dev && njobs > 0 && total_blocks > 0, "pack_weights_batch: bad argument");
    static_assert(sizeof(iswm_pack_job) == 40, "iswm_pack_job layout");
    launch_pack_weights_batch(jobs_dev, njobs, total_blocks, math_planes(conv_math()), (hipStream_t)stream);
    return check_launch("pack_weights_batch");
}

// x: the gathered tensor (forward: x, data gradient: dy), y: the output (y / dx)
static int launch_packed(const iswm_conv_desc* d, bool dgrad, const float* x, const void* wpk, const float* bias, float* y,
                         float* stat_partials, int accumulate, iswm_stream_t stream) {
    const ConvRoute r = plan_route(d, dgrad ? E_DGRAD_PACKED : E_FWD_PACKED, conv_math());
    if (r.family == F_X6_PATCH) {
        PatchArgs p = patch_args(d, dgrad, r.PH, r.PW);
        p.x = x; p.wpk = reinterpret_cast<const uint4*>(wpk); p.bias = bias; p.y = y; p.stats = stat_partials;
        p.accumulate = accumulate;
        launch_conv_x6_patch(p, dgrad, r.planes, (hipStream_t)stream);
        return check_launch(dgrad ? "conv_dgrad_patch" : "conv_fwd_patch");
    }
    ConvArgs a = base_args(d, dgrad);
    a.x = x; a.w = reinterpret_cast<const float*>(wpk); a.bias = bias; a.y = y; a.stats = stat_partials;
    a.accumulate = accumulate;
    ISWM_REQUIRE(launch_conv_x6_pk(a, (hipStream_t)stream, dgrad, r.bm, r.planes), "conv_packed: no kernel for %d-row tiles", r.bm);
    return check_launch(dgrad ? "conv_dgrad_packed" : "conv_fwd_packed");
}

extern "C" int iswm_conv2d_fwd_packed(const iswm_conv_desc* d, const float* x, const void* wpk, const float* bias,
                                      float* y, float* stat_partials, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(x && wpk && y, "conv_fwd_packed: null pointer");
    ISWM_REQUIRE(aligned16(x) && aligned16(wpk) && aligned16(y), "conv_fwd_packed: pointers must be 16-byte aligned");
    ISWM_REQUIRE(d->Cin % 32 == 0, "conv_fwd_packed: Cin must be a multiple of 32");
    return launch_packed(d, false, x, wpk, bias, y, stat_partials, 0, stream);
}

extern "C" int iswm_conv2d_dgrad_packed(const iswm_conv_desc* d, const float* dy, const void* wpk, float* dx,
                                        int accumulate, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(dy && wpk && dx, "conv_dgrad_packed: null pointer");
    ISWM_REQUIRE(aligned16(dy) && aligned16(wpk) && aligned16(dx), "conv_dgrad_packed: pointers must be 16-byte aligned");
    ISWM_REQUIRE(d->Cout % 32 == 0, "conv_dgrad_packed: Cout must be a multiple of 32");
    return launch_packed(d, true, dy, wpk, nullptr, dx, nullptr, accumulate, stream);
}

// ---- activations pre-split into bf16 planes (see include/iswm_hip.h "planes") ----
extern "C" int iswm_split_planes(const float* x, int64_t M, int C, int ldx, void* planes, int ldp, int64_t plane_stride,
                                 iswm_stream_t stream) {
    ISWM_REQUIRE(x && planes && M > 0 && C > 0, "split_planes: bad argument");
    ISWM_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldx >= C && ldp % 4 == 0 && ldp >= C, "split_planes: C %d ldx %d ldp %d", C, ldx, ldp);
    ISWM_REQUIRE(aligned16(x) && plane_stride % 4 == 0 && plane_stride >= M * ldp,
                 "split_planes: planes must be 16-byte aligned and disjoint");
    launch_split_planes(x, M, C, ldx, (unsigned short*)planes, ldp, plane_stride, math_planes(conv_math()), (hipStream_t)stream);
    return check_launch("split_planes");
}

extern "C" int iswm_join_planes(const void* planes, int ldp, int64_t plane_stride, int64_t M, int C, float* x, int ldx,
                                iswm_stream_t stream) {
    ISWM_REQUIRE(x && planes && M > 0 && C > 0, "join_planes: bad argument");
    ISWM_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldx >= C && ldp % 4 == 0 && ldp >= C, "join_planes: C %d ldx %d ldp %d", C, ldx, ldp);
    ISWM_REQUIRE(plane_stride == -1 || plane_stride >= M * ldp, "join_planes: bad plane stride");
    launch_join_planes((const unsigned short*)planes, ldp, plane_stride, M, C, x, ldx, (hipStream_t)stream);
    return check_launch("join_planes");
}

/* second-generation planes kernels (conv_mfma_pl2.hip): kind 0 forward, 1 data gradient */
extern "C" size_t iswm_conv2d_pl2_weight_bytes(const iswm_conv_desc* d, int kind) {
    const int math = conv_math();
    if (!d || math < 1 || (kind != 0 && kind != 1)) return 0;
    const int gc = kind ? d->Cout : d->Cin;
    if (gc % 64 != 0) return 0;
    return packed_weight_bytes_pl2(d->Cout, d->KH * d->KW, d->Cin, kind == 1, math_planes(math));
}

extern "C" int iswm_conv2d_pl2_pack_weights(const iswm_conv_desc* d, int kind, const float* w, void* packed,
                                            iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(kind == 0 || kind == 1, "pl2_pack_weights: kind must be 0 (forward) or 1 (data gradient)");
    ISWM_REQUIRE(w && packed && aligned16(packed), "pl2_pack_weights: bad pointer");
    ISWM_REQUIRE((kind ? d->Cout : d->Cin) % 64 == 0, "pl2_pack_weights: gathered channel count must be a multiple of 64");
    launch_pack_weights_pl2(w, packed, d->Cout, d->KH * d->KW, d->Cin, kind == 1, math_planes(conv_math()), (hipStream_t)stream);
    return check_launch("pl2_pack_weights");
}

// forward (f == nullptr, tiles unused) or data gradient of the planes kernels; xp: planes of the gathered tensor, pitch ldg.
// f: the fused BatchNorm-backward statistics, whose caller allocated `tiles` tile rows
static int launch_pl2(const iswm_conv_desc* d, bool dgrad, const char* what, const void* xp, int ldg, int64_t plane_stride,
                      const void* wpk, const float* bias, float* y, float* stat_partials, int accumulate, const BnFuse* f,
                      int tiles, iswm_stream_t stream) {
    if (int e = validate(d)) return e;
    ISWM_REQUIRE(xp && wpk && y, "%s: null pointer", what);
    ISWM_REQUIRE(aligned16(xp) && aligned16(wpk) && aligned16(y), "%s: pointers must be 16-byte aligned", what);
    const int math = conv_math();
    ISWM_REQUIRE((dgrad ? d->Cout : d->Cin) % 64 == 0 && ldg % 8 == 0 &&
                     (plane_stride % 8 == 0 || (plane_stride == -1 && math_planes(math) == 1)),
                 "%s: gathered channels %% 64, their pitch %% 8, plane stride %% 8 (or -1: one rounded plane under conv math bf16)", what);
    const ConvRoute r = plan_route(d, dgrad ? E_DGRAD_PL2 : E_FWD_PL2, math);
    ISWM_REQUIRE(!f || tiles == r.stat_tiles, "conv_dgrad_pl2_bn: tiles %d != %d", tiles, r.stat_tiles);
    ConvArgs a = base_args(d, dgrad);
    a.x = reinterpret_cast<const float*>(xp); a.w = reinterpret_cast<const float*>(wpk); a.bias = bias; a.y = y;
    a.stats = stat_partials; a.accumulate = accumulate;
    a.xps = plane_stride * 2;
    if (f) a.bnf = *f;
    ISWM_REQUIRE(r.family == F_PL2W ? launch_conv_pl2w(a, (hipStream_t)stream, dgrad, r.planes, r.rbw)
                                    : launch_conv_pl2(a, (hipStream_t)stream, dgrad, r.planes, r.rbw, r.wm),
                 "%s: no kernel for this configuration", what);
    return check_launch(what);
}

extern "C" int iswm_conv2d_fwd_pl2(const iswm_conv_desc* d, const void* xp, int64_t plane_stride, const void* wpk,
                                   const float* bias, float* y, float* stat_partials, iswm_stream_t stream) {
    return launch_pl2(d, false, "conv_fwd_pl2", xp, d ? d->ldx : 0, plane_stride, wpk, bias, y, stat_partials, 0, nullptr, 0, stream);
}

extern "C" int iswm_conv2d_dgrad_pl2(const iswm_conv_desc* d, const void* dyp, int64_t plane_stride, const void* wpk,
                                     float* dx, int accumulate, iswm_stream_t stream) {
    return launch_pl2(d, true, "conv_dgrad_pl2", dyp, d ? d->ldy : 0, plane_stride, wpk, nullptr, dx, nullptr, accumulate, nullptr, 0,
                      stream);
}

/* iswm_conv2d_dgrad_pl2 that also emits, per tile row and input channel, the two sums the BatchNorm backward of the stage
 * that PRODUCED the conv's input needs over the finished dx (after accumulation):  partials[0][t][c] = sum dz,
 * partials[1][t][c] = sum dz * xhat,  dz = dx * [ReLU pattern], xhat = (y - mean) * invstd.  relu: ISWM_GATE_NONE, ISWM_GATE_RECOMPUTED =
 * pattern (y - mean) * mask_scale + mask_shift > 0 (as iswm_bn_backward does), ISWM_GATE_RESIDUAL = the producer is a RESIDUAL stage:
 * pattern = (hi plane of its saved output, mask_hi, pitch ld_mask bf16 elements) > 0, and dx is STORED MASKED (dz): that
 * tensor is both the dout of the producer's BatchNorm backward (call it with ISWM_ACT_NONE) and the gradient of its identity
 * branch, so neither the reduction pass nor a separate `dres` tensor exists for that stage.  y: the producer's raw conv output
 * [N*H*W][ldy], Cin channels.  partials: 2 * tiles * Cin doubles, tiles = iswm_conv2d_dgrad_pl2_stat_tiles(d).  Feed them to
 * iswm_bn_backward_pl with partial_tiles = tiles: it then skips its own reduction pass over dout and y. */
extern "C" int iswm_conv2d_dgrad_pl2_bn(const iswm_conv_desc* d, const void* dyp, int64_t plane_stride, const void* wpk,
                                        float* dx, int accumulate, const float* y, int ldy, const float* mean,
                                        const float* invstd, const float* mask_scale, const float* mask_shift, int relu,
                                        const void* mask_hi, int ld_mask, double* partials, int tiles,
                                        iswm_stream_t stream) {
    ISWM_REQUIRE(d && y && mean && invstd && partials, "conv_dgrad_pl2_bn: null pointer");
    ISWM_REQUIRE(relu == ISWM_GATE_NONE || (relu == ISWM_GATE_RECOMPUTED && mask_scale && mask_shift) ||
                     (relu == ISWM_GATE_RESIDUAL && mask_hi && ld_mask % 4 == 0 && ld_mask >= d->Cin && (((uintptr_t)mask_hi) & 7) == 0),
                 "conv_dgrad_pl2_bn: relu must be 0, 2 (with mask_scale / mask_shift) or 3 (with the producer's saved output planes)");
    ISWM_REQUIRE(d->Cin % 4 == 0 && ldy % 4 == 0 && ldy >= d->Cin && aligned16(y) && aligned16(mean) && aligned16(invstd),
                 "conv_dgrad_pl2_bn: Cin %% 4, ldy %% 4, 16-byte aligned pointers");
    BnFuse f{};
    f.y = y; f.ldy = ldy; f.mean = mean; f.invstd = invstd; f.mscale = mask_scale; f.mshift = mask_shift; f.gate = relu;
    f.part = partials;
    f.mask = reinterpret_cast<const unsigned short*>(mask_hi); f.ldm = ld_mask;
    return launch_pl2(d, true, "conv_dgrad_pl2", dyp, d->ldy, plane_stride, wpk, nullptr, dx, nullptr, accumulate, &f, tiles, stream);
}
