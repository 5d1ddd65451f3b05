// Stand-alone walk of the convolution route planner for host sanitizers (CPU only: every call below is a pure host query, no
// kernel is launched and no device is touched).
//
// Build with the library's sources, host code instrumented, and run on the geometry list of tests/golden/conv_routes.json:
//   python -c "import json; [print(*(v[0] + v[0][3:5])[:11]) for v in json.load(open('tests/golden/conv_routes.json'))['routes'].values()]" > geoms.txt
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc -Xarch_host -fsanitize=address,undefined \
//         tools/route_walk.cpp iswm_amd/csrc/conv_*.hip iswm_amd/csrc/misc.hip -o route_walk
//   ./route_walk geoms.txt
// Each line of the list: n h w cin cout k stride pad dil ldx ldy.  Prints one checksum line per conv math; a sanitizer report
// is the failure.
#include <stdio.h>
#include <string.h>

#include "../include/iswm_hip.h"

static unsigned long long mix(unsigned long long h, unsigned long long v) { return (h ^ v) * 1099511628211ull; }

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: route_walk geoms.txt\n");
        return 2;
    }
    iswm_conv_desc g[512];
    int n = 0, k;
    while (n < 512 && fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d", &g[n].N, &g[n].H, &g[n].W, &g[n].Cin, &g[n].Cout, &k, &g[n].stride,
                             &g[n].pad, &g[n].dil, &g[n].ldx, &g[n].ldy) == 11) {
        iswm_conv_desc& d = g[n++];
        d.KH = d.KW = k;
        d.Ho = (d.H + 2 * d.pad - d.dil * (k - 1) - 1) / d.stride + 1;
        d.Wo = (d.W + 2 * d.pad - d.dil * (k - 1) - 1) / d.stride + 1;
    }
    fclose(f);
    for (int math = 0; math <= 2; ++math) {
        if (iswm_set_conv_math(math)) return 1;
        unsigned long long h = 1469598103934665603ull;
        for (int i = 0; i < n; ++i) {
            const iswm_conv_desc* d = &g[i];
            char name[8];                      // shorter than any kernel name: the formatter must truncate, not overrun
            char full[64];
            for (int kind = 0; kind < 8; ++kind) {
                if (iswm_conv2d_kernel_name(d, kind, name, sizeof(name)) || iswm_conv2d_kernel_name(d, kind, full, sizeof(full))) return 1;
                for (const char* c = full; *c; ++c) h = mix(h, (unsigned char)*c);
            }
            int tiles = 0, rows = 0;
            if (iswm_conv2d_fwd_packed_stat_layout(d, &tiles, &rows)) return 1;
            h = mix(mix(h, tiles), rows);
            h = mix(mix(h, iswm_conv2d_stat_tile_rows(d)), iswm_conv2d_stat_tiles(d));
            for (int kind = 0; kind < 2; ++kind) {
                h = mix(h, iswm_conv2d_packed_weight_bytes(d, kind));
                h = mix(h, iswm_conv2d_pl2_weight_bytes(d, kind));
                h = mix(h, iswm_conv2d_pl2_tile_rows(d, kind));
            }
            h = mix(mix(h, iswm_conv2d_dgrad_pl2_stat_tiles(d)), iswm_conv2d_dgrad_wants_wt(d));
            h = mix(mix(h, iswm_conv2d_wgrad_workspace(d)), iswm_conv2d_wgrad_planes_ok(d));
            h = mix(h, iswm_conv2d_wgrad_planes_workspace(d));
            for (int kind = 0; kind < 4; ++kind) {
                h = mix(h, iswm_packed_weight_bytes(d->Cout, d->KH * d->KW, d->Cin, kind));
                h = mix(h, iswm_pack_job_blocks(d->Cout, d->KH * d->KW, d->Cin, kind));
            }
        }
        printf("conv math %d: %d geometries, checksum %016llx\n", math, n, h);
    }
    return 0;
}
