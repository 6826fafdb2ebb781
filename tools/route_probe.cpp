// route_probe.cpp -- what dsd2dxd_amd/csrc/d2d_route.cpp decides, on the host (tests/test_route_cpu.py).
//   g++ -O2 -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o route_probe route_probe.cpp ...
//       ... ../dsd2dxd_amd/csrc/d2d_route.cpp ../dsd2dxd_amd/csrc/d2d_tables.cpp
//
//   route_probe predicates     "<key> <value>" lines of the lookups and predicates the route is made of (tests/golden/route_predicates.json):
//       shape/<MB>/<N>                        one-group, two-group, fp6 (plain, gain, wide, 2 / 3 / 4 pairs), pipelined int8 (frames, scratch) kernels compiled?
//       poly/<name>                           px_supported, px_groups
//       smem/<filter>/<channels>/<bytes>      mfma_smem_bytes, its waves, mfma2_smem_bytes, its waves
//       pipe/<filter>[.residual]/<channels>/<f|s><layout>/<debug flags>     mfma2_pipelined as a digit (0, 3, 5) for depths 16, 20, 24, 32 x
//                                             dithers T, R, F, X, N x levels 0, -3 dB; f: frames, s: scratch; layout P (planar 4096), I (B = 1),
//                                             2 (il2), M (mono2), C (coop), W (taps32)
//   route_probe                one line per configuration, "<key>\t<field>=<value> ...": every FirRoute field, the predicted kernel name, the main
//                              pass's launch geometry and the fp6 unit, or error=<code>:<text>.  The key is
//                              <dsd_rate>:<output_rate>:<filter>:<channels><fmt><depth><dither>:<level>:<tap_bits>:<kernel>:<debug flags>
//   route_probe keys           the keys of those lines alone, in their order (tools/kernel_instances.py feeds them back through `launches -`)
//   route_probe -              the same lines for the keys on standard input, one per line
//   route_probe launches -     for those keys the launch plans of the engine (d2d_route.h: fir_launch), "<key>\t<pass> <field>=<value> ...[\t<pass> ...]":
//                              the passes it has (main; lo: the residual table's; m2: the mono pair), each with the plan's family, unit, LDS bytes,
//                              waves per block, outputs per wave-tile, wave-tiles per block, grid rows per file and the kernel's name
//   route_probe filters -      for those keys what d2d_filters.h: choose_filters picked and what follows from it at once, "<key>\tfir=<table> M=<decimation>
//                              resamp=<L>/<M>/<P> poly=<table or -> cascade=<0|1> to_scratch=<0|1>", or error=<code>:<text>.  The filter letter of a
//                              key is any d2d_params.filter value: E, X, D, C, or S, the two-stage definition of the 48 kHz multiples
#include <math.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../dsd2dxd_amd/csrc/d2d_route.h"

using namespace d2d;

static const uint32_t DEPTHS[] = {16, 20, 24, 32};
static const char DITHERS[] = {'T', 'R', 'F', 'X', 'N'};
static const double LEVELS[] = {0.0, -3.0};

// ---- predicates: only what the library has always exported, with launch arguments spelled here ----
static FirArgs probe_args(const d2d_filter_def& f, uint32_t ch, uint32_t bits, char dither, double level, bool scratch, char layout, uint32_t dbg) {
    FirArgs a{};
    a.Wb = (uint32_t)(f.ntaps / 8);
    a.B = layout == 'P' || layout == 'M' ? 4096u : 1u;
    a.to_scratch = scratch;
    a.ksteps = (uint32_t)mfma_layout(f.M, f.ntaps).ksteps;
    a.scale_bits = f.S + (layout == 'W' ? 8 : 0);
    a.in_channels = ch;
    a.sum_abs_q = sum_abs_q(f);
    a.mx_exact = mx_exact(f);
    a.il2 = layout == '2'; a.mono2 = layout == 'M'; a.coop = layout == 'C'; a.taps32 = layout == 'W';
    a.dbg_flags = dbg;
    a.epi.gain = pow(10.0, level / 20.0);
    a.epi.scale = bits == 32 ? a.epi.gain : ldexp(a.epi.gain, (int)bits - 1);
    a.epi.bits = bits; a.epi.dither = (uint32_t)dither;
    a.epi.sample_bytes = bits == 16 ? 2 : bits == 32 ? 4 : 3;
    a.epi.channels = ch;
    return a;
}

static void pipe_line(const std::string& name, const d2d_filter_def& f, uint32_t ch, bool scratch, char layout, uint32_t dbg) {
    std::string v;
    for (uint32_t bits : DEPTHS)
        for (char dither : DITHERS)
            for (double level : LEVELS) v += (char)('0' + mfma2_pipelined(probe_args(f, ch, bits, dither, level, scratch, layout, dbg), f.M, f.ntaps));
    printf("pipe/%s/%u/%c%c/%u %s\n", name.c_str(), ch, scratch ? 's' : 'f', layout, dbg, v.c_str());
}

static void predicates() {
    std::vector<int> ns;
    for (const d2d_filter_def& f : D2D_FILTERS) {
        bool seen = false;
        for (int n : ns) seen = seen || n == f.ntaps;
        if (!seen) ns.push_back(f.ntaps);
    }
    for (int MB : {1, 2, 4, 8, 16})
        for (int N : ns) {
            const int M = 8 * MB, NPG = mfma2_pairs(M, N);
            printf("shape/%d/%d one=%d two=%d mx=%d gain=%d wide=%d pairs=%d%d%d%d m3=%d m3scr=%d\n", MB, N, mfma_supported(M, N), mfma2_supported(M, N),
                   mx_supported(MB, N), mx_gain_supported(MB, N), mx_wide_supported(MB, N), mx_pairs_supported(MB, N, 1), mx_pairs_supported(MB, N, 2),
                   mx_pairs_supported(MB, N, 3), mx_pairs_supported(MB, N, 4), mfma3_supported(MB, NPG, N), mfma3_scr_supported(MB, NPG));
        }
    for (const d2d_poly_def& p : D2D_POLYS) printf("poly/%s px=%d groups=%d\n", p.name, px_supported(p), px_groups(p));
    for (const d2d_filter_def& f : D2D_FILTERS)
        for (uint32_t ch = 1; ch <= 8; ++ch)
            for (uint32_t sb = 2; sb <= 4; ++sb) {
                uint32_t w1 = 0, w2 = 0;
                const size_t s1 = mfma_smem_bytes(mfma_layout(f.M, f.ntaps), ch, sb, &w1), s2 = mfma2_smem_bytes(f.M, f.ntaps, ch, sb, &w2);
                printf("smem/%s/%u/%u %zu %u %zu %u\n", f.name, ch, sb, s1, w1, s2, w2);
            }
    const uint32_t DBG[] = {0, D2D_DBG_NO_MX, D2D_DBG_NO_PIPE, D2D_DBG_NO_INTQ, D2D_DBG_NO_GAINQ};
    for (const d2d_filter_def& f : D2D_FILTERS) {
        for (uint32_t dbg : DBG) {
            for (uint32_t ch = 1; ch <= 8; ++ch)
                for (int scratch = 0; scratch < 2; ++scratch)
                    for (char layout : {'P', 'I'}) pipe_line(f.name, f, ch, scratch, layout, dbg);
            for (int scratch = 0; scratch < 2; ++scratch) pipe_line(f.name, f, 2, scratch, '2', dbg);
            pipe_line(f.name, f, 2, false, 'M', dbg);
            pipe_line(f.name, f, 2, false, 'W', dbg);
            for (uint32_t ch : {4u, 8u}) pipe_line(f.name, f, ch, true, 'C', dbg);
        }
        if (!f.half32) continue;
        std::vector<int32_t> half;                   // the second pass of two-pass 32-bit taps: always into the scratch
        const d2d_filter_def lo = residual_def(f, half);
        for (uint32_t ch = 1; ch <= 8; ++ch)
            for (char layout : {'P', 'I'}) pipe_line(std::string(f.name) + ".residual", lo, ch, true, layout, 0);
    }
}

#ifndef ROUTE_PROBE_PREDICATES_ONLY
// ---- routes ----
struct Rate { uint32_t dsd_rate, output_rate; char filter; };
static const Rate RATE_MATRIX[] = {       // tests/test_gpu_parity.py: RATE_MATRIX
    {1, 88200, 'E'}, {1, 176400, 'E'}, {1, 352800, 'E'},
    {2, 88200, 'E'}, {2, 176400, 'E'}, {2, 352800, 'E'}, {2, 705600, 'E'},
    {4, 88200, 'E'}, {4, 176400, 'E'}, {4, 352800, 'E'}, {4, 705600, 'E'}, {4, 1411200, 'E'},
    {8, 352800, 'E'},
    {1, 88200, 'X'}, {1, 176400, 'X'}, {1, 352800, 'X'}, {1, 352800, 'D'},
    {2, 88200, 'C'}, {2, 176400, 'C'}, {2, 352800, 'C'},
    {1, 96000, 'E'}, {1, 192000, 'E'}, {1, 384000, 'E'},
    {2, 96000, 'E'}, {2, 192000, 'E'}, {2, 384000, 'E'},
    {4, 96000, 'E'}, {4, 192000, 'E'}, {4, 384000, 'E'},
    {8, 96000, 'E'},
    // filter 'S', the 48 kHz multiples in two stages: tests/test_cascade_cpu.py, tests/golden/route_cascade.json
    {1, 96000, 'S'}, {1, 192000, 'S'}, {1, 384000, 'S'},
    {2, 96000, 'S'}, {2, 192000, 'S'}, {2, 384000, 'S'},
    {4, 96000, 'S'}, {4, 192000, 'S'}, {4, 384000, 'S'},
    {8, 96000, 'S'},
};

// what choose_filters picked for a key, and the two facts every later decision hangs on: two kernels with a scratch between them or one pass
static void filters_line(const Rate& rt, uint32_t ch, char fmt, uint32_t bits, char dither, double level, uint32_t tap_bits, uint32_t kernel, uint32_t dbg) {
    d2d_params p{};
    p.struct_size = sizeof(p);
    p.dsd_rate = rt.dsd_rate; p.output_rate = rt.output_rate; p.filter = (uint32_t)rt.filter; p.channels = ch;
    p.fmt = fmt == 'P' ? D2D_FMT_PLANAR : D2D_FMT_INTERLEAVED; p.endianness = fmt == 'P' ? D2D_LSB_FIRST : D2D_MSB_FIRST; p.block_size = 4096;
    p.bit_depth = bits; p.dither = (uint32_t)dither; p.level_db = level; p.seed = 7; p.tap_bits = tap_bits; p.kernel = kernel; p.debug_flags = dbg;
    printf("%u:%u:%c:%u%c%u%c:%d:%u:%u:%u\t", rt.dsd_rate, rt.output_rate, rt.filter, ch, fmt, bits, dither, (int)level, tap_bits, kernel, dbg);
    FilterChoice fc; FirRoute r; std::string err;
    int rc = choose_filters(p, fc, err);
    if (rc == D2D_OK) rc = choose_route(p, fc, r, err);
    if (rc != D2D_OK) { printf("error=%d:%s\n", rc, err.c_str()); return; }
    const FirArgs a = fir_args_static(p, fc, epilogue_of(p), r);
    printf("fir=%s M=%d resamp=%d/%d/%d poly=%s cascade=%d to_scratch=%u\n", fc.fir->name, fc.fir->M, fc.resamp ? fc.resamp->L : 0, fc.resamp ? fc.resamp->Mdn : 0,
           fc.resamp ? fc.resamp->P : 0, fc.poly ? fc.poly->name : "-", fc.resamp && !fc.poly, a.to_scratch);
}

static void launch_field(const char* pass, const FirLaunch& l) {
    printf("\t%s family=%d unit=%d lds=%zu nwaves=%u tile=%u block_tiles=%u rows=%u name=%s", pass, l.family, l.unit, l.lds, l.nwaves, l.tile, l.block_tiles,
           l.rows_per_file, l.name.c_str());
}

static bool keys_only = false;       // `route_probe keys`: the sweep's keys and nothing about them

static void route_line(const Rate& rt, uint32_t ch, char fmt, uint32_t bits, char dither, double level, uint32_t tap_bits, uint32_t kernel, uint32_t dbg,
                       bool launches = false) {
    d2d_params p{};
    p.struct_size = sizeof(p);
    p.dsd_rate = rt.dsd_rate; p.output_rate = rt.output_rate; p.filter = (uint32_t)rt.filter; p.channels = ch;
    p.fmt = fmt == 'P' ? D2D_FMT_PLANAR : D2D_FMT_INTERLEAVED; p.endianness = fmt == 'P' ? D2D_LSB_FIRST : D2D_MSB_FIRST; p.block_size = 4096;
    p.bit_depth = bits; p.dither = (uint32_t)dither; p.level_db = level; p.seed = 7; p.tap_bits = tap_bits; p.kernel = kernel; p.debug_flags = dbg;
    printf("%u:%u:%c:%u%c%u%c:%d:%u:%u:%u%c", rt.dsd_rate, rt.output_rate, rt.filter, ch, fmt, bits, dither, (int)level, tap_bits, kernel, dbg, keys_only ? '\n' : '\t');
    if (keys_only) return;
    FilterChoice fc; FirRoute r; std::string err;
    int rc = choose_filters(p, fc, err);
    if (rc == D2D_OK) rc = choose_route(p, fc, r, err);
    if (rc != D2D_OK) { printf("error=%d:%s\n", rc, err.c_str()); return; }
    const Epilogue epi = epilogue_of(p);
    if (launches) {
        printf("ok");
        launch_field("main", fir_launch(p, fc, epi, r, PASS_MAIN));
        if (r.fine) {
            std::vector<int32_t> half;
            const d2d_filter_def lo = residual_def(*fc.fir, half);
            launch_field("lo", fir_launch(p, fc, epi, r, PASS_LO, &lo));
        }
        if (r.mono2_pipe != PIPE_NONE) launch_field("m2", fir_launch(p, fc, epi, r, PASS_MONO2));
        printf("\n");
        return;
    }
    printf("kernel=%u poly=%d poly_plain=%d mfma_v2=%d mfma_pipe=%d mfma_pipe_lo=%d fine=%d taps32=%d deinterleave=%d il2=%d coop=%d B=%u keep=%u mono2_pipe=%d "
           "table_variant=%u variant=%u", r.kernel, r.poly, r.poly_plain, r.mfma_v2, r.mfma_pipe, r.mfma_pipe_lo, r.fine, r.taps32, r.deinterleave, r.il2,
           r.coop, r.B, r.keep, r.mono2_pipe, r.table_variant, route_table_variant(r));
    if (!r.poly && r.kernel == D2D_KERNEL_MFMA) {
        const d2d_filter_def& f = *fc.fir;
        const FirArgs a = fir_args_static(p, fc, epi, r);
        size_t smem = 0;
        if (r.mfma_v2) {
            // (the LDS bytes and the waves of the two-group geometry, whichever kernel serves; what the fp6 kernel's plan makes of gainq and the pairs)
            Mfma2Args m{};
            mfma2_geometry(a, f.M / 8, mfma2_pairs(f.M, f.ntaps), m, smem);
            const FirLaunch l = fir_launch(p, fc, epi, r, PASS_MAIN);
            const bool mx = l.family == FIR_MX;
            printf(" lds=%zu nwaves=%u ngroups=%u intq=%u gainq=%u wide=%u epilogue=%d npairs=%u mx_unit=%d", smem, m.nwaves, m.ngroups, m.intq, mx ? l.m.gainq : m.gainq,
                   m.wide, mfma2_epilogue(a, m), mx ? l.m.npairs : m.npairs, mx ? l.unit : -1);
        } else {
            MfmaArgs m{};
            mfma_geometry(a, mfma_layout(f.M, f.ntaps), m, smem);
            printf(" lds=%zu nwaves=%u ngroups=%u wide=%u", smem, m.nwaves, m.ngroups, m.wide);
        }
    }
    printf(" name=%s\n", route_kernel_name(r, fc, epi).c_str());       // (last: the name holds blanks)
}

static void routes() {
    const uint32_t FLAGS[] = {D2D_DBG_NO_COOP, D2D_DBG_NO_MX, D2D_DBG_NO_PIPE, D2D_DBG_MFMA_V1, D2D_DBG_TAPS32_2PASS, D2D_DBG_NO_INTQ, D2D_DBG_NO_GAINQ};
    for (const Rate& rt : RATE_MATRIX)
        for (char fmt : {'P', 'I'})
            for (uint32_t bits : DEPTHS)
                for (char dither : DITHERS)
                    for (double level : LEVELS)
                        for (uint32_t tap_bits : {0u, 24u, 32u})
                            for (uint32_t kernel : {0u, 1u, 2u}) {
                                for (uint32_t ch = 1; ch <= 8; ++ch) route_line(rt, ch, fmt, bits, dither, level, tap_bits, kernel, 0);
                                for (uint32_t flag : FLAGS) route_line(rt, 2, fmt, bits, dither, level, tap_bits, kernel, flag);      // the diagnostic routes, on stereo
                            }
}
#endif

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "predicates") { predicates(); return 0; }
#ifndef ROUTE_PROBE_PREDICATES_ONLY
    keys_only = argc > 1 && std::string(argv[1]) == "keys";
    if (argc == 1 || keys_only) { routes(); return 0; }
    const bool launches = std::string(argv[1]) == "launches", filters = std::string(argv[1]) == "filters";
    if (std::string(argv[(launches || filters) && argc > 2 ? 2 : 1]) == "-") {
        Rate rt; unsigned ch, bits, tap_bits, kernel, dbg; int level; char fmt, dither;
        while (scanf("%u:%u:%c:%u%c%u%c:%d:%u:%u:%u", &rt.dsd_rate, &rt.output_rate, &rt.filter, &ch, &fmt, &bits, &dither, &level, &tap_bits, &kernel, &dbg) == 11)
            if (filters) filters_line(rt, ch, fmt, bits, dither, level, tap_bits, kernel, dbg);
            else route_line(rt, ch, fmt, bits, dither, level, tap_bits, kernel, dbg, launches);
        return 0;
    }
#endif
    fprintf(stderr, "usage: route_probe [predicates | keys | - | launches - | filters -]\n");
    return 2;
}
