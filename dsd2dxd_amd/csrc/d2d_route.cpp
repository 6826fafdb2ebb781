// d2d_route.cpp -- see d2d_route.h.  Host code only; the conditions are the ones d2d_create and the launchers have always applied, in their order.
#include "d2d_route.h"

#include <math.h>
#include <stdlib.h>

namespace d2d {

// ---- the compiled kernels: every lookup reads its unit list and nothing else --------------------------------------------------------
int mx_find(int MB, int NT, MxFlavour fl, int npr) {
#define X(unit, mb, nt, f, n) if (mx_unit_kept(mb, nt) && MB == mb && NT == nt && fl == f && npr == n) return unit;
    D2D_MX_UNIT_LIST(X)
#undef X
    return -1;
}
bool mx_supported(int MB, int NT) { return mx_find(MB, NT, MX_INT, 1) >= 0; }
bool mx_pairs_supported(int MB, int NT, int npairs) { return npairs > 1 && mx_find(MB, NT, MX_INT, npairs) >= 0; }
bool mx_wide_supported(int MB, int NT) { return mx_find(MB, NT, MX_WIDE, 1) >= 0; }
bool mx_gain_supported(int MB, int NT) { return mx_find(MB, NT, MX_GAIN, 1) >= 0; }
int mx_groups(int MB) { return mx_g(MB); }

// the unit of a shape (one at most), and whether it serves frames with NT taps
int m3_find(int MB, int NPG) {
#define X(unit, mb, npg, nt0, nt1) if (m3_unit_kept(mb, npg) && MB == mb && NPG == npg) return unit;
    D2D_M3_UNIT_LIST(X)
#undef X
    return -1;
}
bool m3_frames(int u, int NT) {
#define X(unit, mb, npg, nt0, nt1) if (u == unit) return NT > 0 && (nt0 == NT || nt1 == NT);
    D2D_M3_UNIT_LIST(X)
#undef X
    return false;
}
bool mfma3_scr_supported(int MB, int NPG) { return m3_find(MB, NPG) >= 0; }
bool mfma3_supported(int MB, int NPG, int NT) { return m3_frames(m3_find(MB, NPG), NT); }

int px_find(const d2d_poly_def& p) {
#define X(unit, lp, mp, np, g) if (p.Lp == lp && p.Mp == mp && p.NP == np) return unit;
    D2D_PX_UNIT_LIST(X)
#undef X
    return -1;
}
bool px_supported(const d2d_poly_def& p) { return px_find(p) >= 0; }

bool mfma_supported(int M, int N) {
    (void)N;
    return M == 8 || M == 16 || M == 32 || M == 64 || M == 128;
}

bool mfma2_supported(int M, int N) {
    const int MB = M / 8, NPG = mfma2_pairs(M, N);
#define X(mb, npg) if (MB == mb && NPG == npg) return true;
    D2D_M2_SHAPES(X)
#undef X
    return false;
}

// the waves of a block before LDS has its say: the diagnostic override (d2d_params.debug_flags bits 8..15) or `most`
static uint32_t waves_asked(const FirArgs& a, uint32_t most) {
    const uint32_t wdbg = (a.dbg_flags >> 8) & 0xFFu;
    return wdbg < 1 || wdbg > most ? most : wdbg;
}

// ---- the one-group kernel's geometry ---------------------------------------------------------------------------------------------
void mfma_geometry(const FirArgs& a, const MfmaLayout& g, MfmaArgs& m, size_t& smem) {
    // channels per block: all of a mono/stereo file, one pair of a multichannel one
    m.ngroups = a.epi.channels <= 2 ? 1u : (a.epi.channels + 1u) / 2u;
    const uint32_t C = a.epi.channels <= 2 ? a.epi.channels : 2u;
    const int MB = g.M / 8;
    m.f = a;
    m.c0 = a.to_scratch ? ldexp(1.0, a.scale_bits) : (a.epi.bits == 32 ? a.epi.gain : a.epi.scale);   // scratch: the integer y*2^S
    m.c1 = ldexp(m.c0, 1 - a.scale_bits - 7);     // exact: a power-of-two multiple of c0
    m.dsel = a.epi.dither == 'T' ? 1u : 0u;
    m.dkind = a.epi.dither == 'T' ? 1u : (a.epi.dither == 'R' ? 2u : 0u);
    m.dmul = a.epi.dither == 'T' ? 0x1p-16 : (a.epi.dither == 'R' ? 0x1p-17 : 0.0);
    m.dadd = a.epi.dither == 'T' ? -1.0 : (a.epi.dither == 'R' ? -0.5 : 0.0);
    m.qsh = a.epi.bits == 20 ? 4u : 0u;
    m.qmin_i = a.epi.bits == 32 ? 0 : -(1 << (a.epi.bits - 1)); m.qmax_i = a.epi.bits == 32 ? 0 : (1 << (a.epi.bits - 1)) - 1;
    m.U = (uint32_t)g.ksteps / 2;
    // |limb sum| <= (bytes of row window) * 255 * 128; below 2^23 the pairs recombine in int32
    m.wide = (uint64_t)g.ksteps * 4u * 255u * 128u >= (1u << 23) ? 1u : 0u;
    int ls = 0;
    while ((1 << ls) < 2 * MB) ++ls;
    m.ls = (uint32_t)ls;
    // logical staged bytes per channel: 16-byte alignment slack + 31 row strides + one row window
    // (+3 dwords read ahead) + slack for the in-register byte realignment
    m.span = (16u + 31u * 8u * MB + (2 * m.U + 5) * 4u + 16u + 15u) & ~15u;
    const uint32_t ldw = m.span / 4;
    m.ppair = ((2u * (ldw + (ldw >> ls) + 2u)) * 4u + 15u) & ~15u;
    m.off_waves = ((uint32_t)g.ksteps + 6u) * 1024u + 64u;   // + MFMA-phase tokens
    m.off_out = ((C + 1) / 2) * m.ppair;
    m.off_pk = m.off_out + ((256u * C * a.epi.sample_bytes + 15u) & ~15u);
    m.wave_lds = m.off_pk + C * 64u * 8u + ((C * 16u + 15u) & ~15u);   // peaks + per-channel dither keys
#if D2D_DIAG
    { static const char* e = getenv("D2D_DBG"); m.dbg = e ? (uint32_t)atoi(e) : 0u; }          // (make DIAG=1 builds only: never the shipped library)
    { static const char* e = getenv("D2D_STAGGER"); m.stagger = e ? (uint32_t)atoi(e) : 0u; }
#endif
    m.nwaves = waves_asked(a, 12);
    // largest block that fits the CU's LDS, keeping the waves evenly spread over the four SIMDs
    while (m.nwaves > 1 && (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds > 160 * 1024)
        m.nwaves = m.nwaves > 8 ? 8 : m.nwaves > 4 ? 4 : m.nwaves >> 1;
    smem = (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds;
}

size_t mfma_smem_bytes(const MfmaLayout& g, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block) {
    FirArgs a{};
    a.epi.channels = channels; a.epi.sample_bytes = sample_bytes; a.epi.bits = 24;
    MfmaArgs m{}; size_t smem = 0;
    mfma_geometry(a, g, m, smem);
    if (waves_per_block) *waves_per_block = m.nwaves;
    return smem;
}

// ---- the two-group kernels -------------------------------------------------------------------------------------------------------

// the epilogue flavour of a launch: 2 = the integers for the stage-A scratch, 1 = stereo 24-bit packed in registers, 0 = anything via LDS
int mfma2_epilogue(const FirArgs& a, const Mfma2Args& m) {
    if (a.to_scratch) return 2;
    return a.epi.channels == 2 && a.epi.sample_bytes == 3 && m.qsh == 0 && !m.wide ? 1 : 0;
}

// the pipelined kernel serves the register-packed stereo flavour with the all-integer requantiser; its accumulators start
// from -2^(S-18) in the limb-3 rows
static bool mfma3_eligible(const FirArgs& a, const Mfma2Args& m, int MB, int NPG, int NT) {
    // stereo, 24-bit packed or 16-bit frames, the all-integer requantiser (unit gain)
    // the exact integers for the stage-A scratch: every channel pair of an even channel count
    if (a.to_scratch) return a.epi.channels >= 2 && a.epi.channels % 2 == 0 && !m.wide && a.scale_bits >= 18 && a.scale_bits <= 30 &&
                             a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31) && mfma3_scr_supported(MB, NPG);
    const bool frames_ok = a.epi.channels == 2 && (a.epi.sample_bytes == 3 || a.epi.sample_bytes == 2) && m.qsh == 0 && !m.wide;
    const bool shape_ok = a.scale_bits >= 18 && a.scale_bits <= 30 && mfma3_supported(MB, NPG, NT);
    // ... or 32-bit float at 0 dB without the float dither: the sample is (float)v * 2^-S
    const bool noint = (a.dbg_flags & D2D_DBG_NO_INTQ) != 0;
    const bool float_ok = !noint && a.epi.channels == 2 && a.epi.bits == 32 && a.epi.dither != 'F' && a.epi.gain == 1.0 && !m.wide &&
                          a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31);
    // (M = 8 float frames too since the pipelined kernel stages that shape's frames through LDS: 4.18 against 4.50 ms on the one-group kernel)
    if (float_ok && shape_ok) return true;
    if (m.gainq && shape_ok && MB < 4) return true;            // another level in dB, M = 8 and 16: the f64 requantiser inside the pipelined epilogue
    return frames_ok && m.intq && shape_ok;
}

// Planar frames of an even channel count above two on the fp6 kernel: a wave converts every pair of a tile and stores whole frames
// (d2d_kernels_mx.hip, NPR).  The pairs per wave, or 1.  (Byte-interleaved multichannel input reaches the kernel as the engine's planar copy.)
static uint32_t mx_pairs(const FirArgs& a, int MB, int N) {
    const uint32_t C = a.epi.channels;
    if (a.to_scratch || a.mono2 || a.il2 || a.coop || C < 4 || C % 2) return 1u;
    if (a.B < 16 || (a.B & (a.B - 1)) != 0) return 1u;
    return mx_pairs_supported(MB, N, (int)(C / 2u)) ? C / 2u : 1u;
}

// the tables whose digit sums the fp6 kernel recombines exactly, with v = sum q s in an int32
static bool mx_range_ok(const FirArgs& a) {
    return a.scale_bits >= 20 && a.scale_bits <= 30 && a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31) && a.mx_exact;
}

// the same conversions as mfma3_eligible, shape apart (the caller checks mx_supported)
static bool mx_eligible(const FirArgs& a, const Mfma2Args& m, int MB, int N) {
    const bool range_ok = mx_range_ok(a);
    if (a.to_scratch) return a.epi.channels >= 2 && a.epi.channels % 2 == 0 && range_ok;
    const bool noint = (a.dbg_flags & D2D_DBG_NO_INTQ) != 0;
    const bool stereo = (a.epi.channels == 2 || mx_pairs(a, MB, N) > 1u) && m.qsh == 0;       // (or whole frames of several pairs)
    const bool float_ok = !noint && stereo && a.epi.bits == 32 && a.epi.dither != 'F' && a.epi.gain == 1.0;
    const bool frames_ok = stereo && (a.epi.sample_bytes == 3 || a.epi.sample_bytes == 2) && m.intq;
    return range_ok && (float_ok || frames_ok);
}

int mfma2_pipelined(const FirArgs& a, int M, int N) {
    if (a.taps32) return PIPE_FP6;                            // (the engine has checked mx_wide_supported and mx_wide_exact)
    if (a.dbg_flags & D2D_DBG_NO_PIPE) return PIPE_NONE;
    const int MB = M / 8, NPG = mfma2_pairs(M, N);
    const bool nomx = (a.dbg_flags & D2D_DBG_NO_MX) != 0;
    Mfma2Args m{}; size_t smem = 0;
    mfma2_geometry(a, MB, NPG, m, smem);
    // M = 128 (DSD256 -> 88.2 kHz, DSD512 -> 176.4 kHz): only the fp6 kernel has the LDS for that tap table; its conditions are its own
    // (S = 30: no biased accumulators, and the int8 kernels' limb-sum bound `wide` does not apply)
    if (MB == 16) {
        const bool noint16 = (a.dbg_flags & D2D_DBG_NO_INTQ) != 0;
        if (nomx || !mx_supported(MB, N) || !mx_range_ok(a) || noint16) return PIPE_NONE;
        if (a.to_scratch) return a.epi.channels >= 2 && a.epi.channels % 2 == 0 ? PIPE_FP6 : PIPE_NONE;
        const bool depth_ok = a.epi.bits == 32 ? true : ((a.epi.bits == 24 || a.epi.bits == 20 || a.epi.bits == 16) && m.fbits > 0 && m.fbits <= 16 && a.epi.dither != 'F');
        const bool mp = mx_pairs(a, MB, N) > 1u;
        if ((a.epi.channels != 2 && !mp) || !depth_ok || a.epi.dither == 'N') return PIPE_NONE;
        if (a.epi.gain == 1.0 && m.qsh == 0 && !(a.epi.bits == 32 && a.epi.dither == 'F')) return PIPE_FP6;
        if (mp) return PIPE_NONE;                                  // (several pairs per wave: unit gain only)
        return mx_gain_supported(MB, N) && !(a.dbg_flags & D2D_DBG_NO_GAINQ) ? PIPE_FP6 : PIPE_NONE;
    }
    // the fp6 x fp4 kernel (d2d_kernels_mx.hip) serves what the pipelined int8 kernel serves at M = 32 and 64
    if (!nomx && mx_supported(MB, N) && mx_eligible(a, m, MB, N)) return PIPE_FP6;
    // ... and stereo frames at another level than 0 dB (its gain flavours; gainq has tested sum_abs_q already)
    if (!nomx && m.gainq && mx_gain_supported(MB, N) && mx_range_ok(a) && (a.epi.bits == 32 || a.epi.sample_bytes == 2 || a.epi.sample_bytes == 3)) return PIPE_FP6;
    if (!mfma2_supported(M, N) && !mfma3_supported(MB, NPG, N) && !(a.to_scratch && mfma3_scr_supported(MB, NPG))) return PIPE_NONE;
    if (!mfma3_eligible(a, m, MB, NPG, N)) return PIPE_NONE;
    return PIPE_INT8;
}

void mfma2_geometry(const FirArgs& a, int MB, int NPG, Mfma2Args& m, size_t& smem) {
    m.ngroups = a.epi.channels <= 2 ? 1u : (a.epi.channels + 1u) / 2u;
    m.npairs = 1u;
    const uint32_t C = a.epi.channels <= 2 ? a.epi.channels : 2u;
    m.f = a;
    m.c0 = a.to_scratch ? ldexp(1.0, a.scale_bits) : (a.epi.bits == 32 ? a.epi.gain : a.epi.scale);   // scratch: the integer y*2^S
    m.c1 = ldexp(m.c0, 1 - a.scale_bits - 7);     // exact: a power-of-two multiple of c0
    m.dkind = a.epi.dither == 'T' ? 1u : (a.epi.dither == 'R' ? 2u : 0u);
    m.dmul = a.epi.dither == 'T' ? 0x1p-16 : (a.epi.dither == 'R' ? 0x1p-17 : 0.0);
    m.dadd = a.epi.dither == 'T' ? -1.0 : (a.epi.dither == 'R' ? -0.5 : 0.0);
    m.qsh = a.epi.bits == 20 ? 4u : 0u;
    m.qmin_i = a.epi.bits == 32 ? 0 : -(1 << (a.epi.bits - 1)); m.qmax_i = a.epi.bits == 32 ? 0 : (1 << (a.epi.bits - 1)) - 1;
    // |limb sum| <= (bytes of a group's window) * 255 * 128; below 2^23 the pairs recombine in int32
    m.wide = m2_unmask0(NPG) ? 0u : ((uint64_t)NPG * 8u * 255u * 128u >= (1u << 23) ? 1u : 0u);
    m.fbits = a.scale_bits - ((int)a.epi.bits - 1);
    const bool noint = (a.dbg_flags & D2D_DBG_NO_INTQ) != 0;
    // (the fast form carries v0 = v + 2^S in an int32: 2^S + sum|q| has to stay below 2^31)
    m.intq = (!noint && !a.to_scratch && a.epi.bits != 32 && a.epi.gain == 1.0 && !m.wide && m.fbits > 0 && m.fbits <= 16 &&
              a.sum_abs_q != 0 && (1ull << a.scale_bits) + a.sum_abs_q < (1ull << 31)) ? 1u : 0u;
    // stereo 16/24-bit (dither T, R, none) or float (no float dither) frames at another level than 0 dB, and 20-bit frames and the float dither (the CLI's default for -b 32) at any level
    // (the all-integer requantiser has no 20-in-24 form; the f64 one shifts its result)
    m.gainq = (!noint && !(a.dbg_flags & D2D_DBG_NO_GAINQ) && !a.to_scratch && a.epi.channels == 2 && (a.epi.gain != 1.0 || m.qsh != 0 || (a.epi.bits == 32 && a.epi.dither == 'F')) && !m.wide &&
               (a.epi.dither != 'F' || a.epi.bits == 32) && a.epi.dither != 'N' && (a.epi.bits == 32 || (m.fbits > 0 && m.fbits <= 16)) && a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31)) ? 1u : 0u;
    m.off_waves = (uint32_t)(2 * NPG) * 1024u;
    m.off_out = (uint32_t)m2_stream_bytes(MB, NPG);
    // (only the LDS-staged epilogue needs the output slice)
    const bool lds_out = mfma2_epilogue(a, m) == 0;
    m.wave_lds = m.off_out + (lds_out ? (((uint32_t)M2_TILE * C * a.epi.sample_bytes + 15u) & ~15u) : 0u);
#if D2D_DIAG
    { static const char* e = getenv("D2D_DBG"); m.dbg = e ? (uint32_t)atoi(e) : 0u; }     // (make DIAG=1 builds only: never the shipped library)
#endif
    m.nwaves = waves_asked(a, 12);
    // largest block that fits the CU's LDS, keeping the waves evenly spread over the four SIMDs
    while (m.nwaves > 1 && (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds > 160 * 1024)
        m.nwaves = m.nwaves > 8 ? 8 : m.nwaves > 4 ? 4 : m.nwaves >> 1;
    smem = (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds;
}

size_t mfma2_smem_bytes(int M, int N, uint32_t channels, uint32_t sample_bytes, uint32_t* waves_per_block) {
    FirArgs a{};
    a.epi.channels = channels; a.epi.sample_bytes = sample_bytes; a.epi.bits = 24;
    Mfma2Args m{}; size_t smem = 0;
    mfma2_geometry(a, M / 8, mfma2_pairs(M, N), m, smem);
    if (waves_per_block) *waves_per_block = m.nwaves;
    return smem;
}

// ---- the route -------------------------------------------------------------------------------------------------------------------

Epilogue epilogue_of(const d2d_params& p) {
    Epilogue epi{};
    epi.gain = pow(10.0, p.level_db / 20.0);
    epi.scale = p.bit_depth == 32 ? epi.gain : ldexp(epi.gain, (int)p.bit_depth - 1);
    epi.seed = p.seed;
    epi.bits = p.bit_depth;
    epi.dither = p.dither;
    if (p.dither == 'N' && p.bit_depth == 32) epi.dither = 'X';                     // float output: nothing to shape
    epi.sample_bytes = p.bit_depth == 16 ? 2 : (p.bit_depth == 32 ? 4 : 3);
    epi.channels = p.channel_count ? p.channel_count : p.channels - p.channel_first;
    return epi;
}

d2d_params mix_fir_params(const d2d_params& p) {
    d2d_params q = p;
    q.dither = D2D_DITHER_NOISE_SHAPED;
    if (q.bit_depth == 32) q.bit_depth = 24;
    return q;
}

// a halved engine's FIR pass: the 'N' dither's integer pass of twice the final rate (every kernel it reaches is one the unhalved engine of
// that rate reaches)
d2d_params half_fir_params(const d2d_params& p) {
    d2d_params q = mix_fir_params(p);
    q.output_rate = p.output_rate * 2u;
    return q;
}

FirArgs fir_args_static(const d2d_params& p, const FilterChoice& fc, const Epilogue& epi, const FirRoute& r, const d2d_filter_def* lo) {
    const d2d_filter_def& f = *fc.fir;
    const d2d_filter_def& fd = lo ? *lo : f;
    const LutLayout lut = lut_layout(f.M / 8, f.ntaps / 8);
    const bool cascade = fc.resamp && !fc.poly, noise_shape = epi.dither == 'N';
    FirArgs a{};
    a.Wb = (uint32_t)(f.ntaps / 8);
    a.ntab = (uint32_t)lut.ntab; a.pad = (uint32_t)lut.pad; a.nq = (uint32_t)lut.nq;
    a.B = r.B; a.keep = r.keep;
    a.to_scratch = (cascade || noise_shape || r.fine) ? 1u : 0u;
    a.ksteps = (uint32_t)mfma_layout(f.M, f.ntaps).ksteps;
    a.scale_bits = f.S + (r.taps32 ? 8 : 0);
    a.taps32 = r.taps32 ? 1u : 0u;
    a.in_channels = p.channels;
    a.sum_abs_q = sum_abs_q(fd);
    a.epi = epi;
    a.pipelined = (uint32_t)(lo ? r.mfma_pipe_lo : r.mfma_pipe);
    a.mx_exact = mx_exact(fd) ? 1u : 0u;
    a.coop = r.coop ? 1u : 0u;
    a.il2 = r.il2 ? 1u : 0u;
    a.dbg_flags = p.debug_flags;
    return a;
}

uint32_t route_table_variant(const FirRoute& r) {
    if (r.taps32) return 8u;      // the seven-digit fragments of the 32-bit taps
    return r.poly ? (r.poly_plain ? 7u : 6u) : r.kernel == D2D_KERNEL_MFMA && r.mfma_v2 ? (r.mfma_pipe ? (uint32_t)r.mfma_pipe : 2u) : 0u;
}

int choose_route(const d2d_params& p, const FilterChoice& fc, FirRoute& r, std::string& err) {
    r = FirRoute{};
    const d2d_filter_def& f = *fc.fir;
    const int M = f.M, Mb = f.M / 8, N = f.ntaps, Wb = f.ntaps / 8;
    const Epilogue epi = epilogue_of(p);
    const uint32_t Cin = p.channels, C = epi.channels;
    const bool noise_shape = epi.dither == 'N';
    auto fail = [&err](const char* m) { err = m; return D2D_ERR_PARAM; };
    r.B = p.fmt == D2D_FMT_INTERLEAVED ? 1u : p.block_size;   // README.md:9
    if (r.B == 1) {   // byte interleaved: mono is already planar; otherwise a planar copy is made per call
        r.deinterleave = Cin > 1;
        r.B = 4096;
    }
    if (p.tap_bits != 0 && p.tap_bits != 24 && p.tap_bits != 32) return fail("Invalid tap grid; must be 24 or 32 bits");
    if (p.tap_bits == 32) {
        if (fc.resamp || noise_shape) return fail("32-bit taps serve the 44.1k-family rates with dither T, R, F or X");
        r.fine = true;
    }
    r.poly = fc.poly != nullptr;
    const MfmaLayout mfma = mfma_layout(M, N);
    uint32_t mfma_waves = 0;
    bool mfma_ok = mfma_supported(M, N) &&
                   mfma_smem_bytes(mfma, C, epi.sample_bytes, &mfma_waves) <= 160 * 1024;
    {   // the two-group kernel wherever its shape is compiled and four waves fit in LDS (D2D_MFMA_V1=1: the older one)
        const bool v1 = (p.debug_flags & D2D_DBG_MFMA_V1) != 0;
        uint32_t w2 = 0;
        if (!v1 && mfma2_supported(M, N) &&
            mfma2_smem_bytes(M, N, C, epi.sample_bytes, &w2) <= 160 * 1024 && w2 >= 4) {
            r.mfma_v2 = true; mfma_ok = true; mfma_waves = w2;
        }
        // M = 8 and 16: the two-group geometry only through the pipelined kernel (stereo 16/24-bit/float frames at 0 dB); every other
        // format of those rates stays on the one-group kernel
        if (!v1 && !r.mfma_v2 && (M < 32 || M == 128) && p.kernel != D2D_KERNEL_LUT) {
            if (mfma2_pipelined(fir_args_static(p, fc, epi, r), M, N)) { r.mfma_v2 = true; mfma_ok = true; mfma_waves = 8; }
        }
    }
    // AUTO: the matrix-core kernel whenever a full 4-wave block fits in LDS (it works per channel pair,
    // so only an extremely long window can fail this; then the LUT kernel)
    r.kernel = p.kernel == D2D_KERNEL_AUTO ? (mfma_ok && mfma_waves >= 4 ? D2D_KERNEL_MFMA : D2D_KERNEL_LUT) : p.kernel;
    if (r.poly) {
        // the matrix-core form wherever a kernel is compiled for the table and its digit sums are exact in f32 (all six shipped tables)
        const bool px_ok = px_supported(*fc.poly) && px_exact(*fc.poly);
        r.kernel = p.kernel == D2D_KERNEL_AUTO ? (px_ok ? D2D_KERNEL_MFMA : D2D_KERNEL_LUT) : p.kernel;
        mfma_ok = px_ok;
        r.poly_plain = r.kernel == D2D_KERNEL_LUT;
        r.mfma_v2 = false;
    }
    if (r.kernel == D2D_KERNEL_MFMA && !mfma_ok)
        return fail("MFMA kernel does not support this configuration (decimation or LDS budget)");
    r.keep = (uint32_t)(Wb + Mb);
    // (direct polyphase: the oldest bit an output of the next call can need lies NP - D + M bits before the call's first byte)
    if (r.poly) r.keep = std::max<uint32_t>(r.keep, (uint32_t)((fc.poly->NP - fc.poly->D + M + 7) / 8 + 2));
    r.keep = (r.keep + 15u) & ~15u;

    if (r.poly) {
        // byte-interleaved stereo (DFF files, the CLI's default -f I): de-interleaved inside the kernel's staging, no planar copy (D2D_NO_COOP=1: the pre-pass)
        if (!r.poly_plain && r.deinterleave && Cin == 2 && C == 2 && !(p.debug_flags & D2D_DBG_NO_COOP)) { r.il2 = true; r.deinterleave = false; r.B = 1; }
    } else if (r.kernel != D2D_KERNEL_LUT) {
        // 32-bit taps in ONE pass where the fp6 kernel's seven-digit flavour is compiled for the table and its digit sums are exact: stereo frames,
        // any depth, dither and level (D2D_DBG_TAPS32_2PASS: the two scratch passes and the combining pass, which serve everything else)
        if (r.fine && r.mfma_v2 && C == 2 && Cin == 2 && mx_wide_supported(M / 8, N) && mx_wide_exact(f) &&
            !(p.debug_flags & (D2D_DBG_TAPS32_2PASS | D2D_DBG_NO_MX | D2D_DBG_NO_PIPE | D2D_DBG_MFMA_V1 | D2D_DBG_NO_GAINQ))) {
            r.fine = false; r.taps32 = true;
        }
        if (r.mfma_v2) r.mfma_pipe = mfma2_pipelined(fir_args_static(p, fc, epi, r), M, N);
        // byte-interleaved 4- or 8-channel input into the scratch (48k family, noise shaping) through the fp6 kernel: no planar copy, the
        // kernel's staging de-interleaves (D2D_DBG_NO_COOP: the pre-pass)
        {
            const bool nocoop = (p.debug_flags & D2D_DBG_NO_COOP) != 0;
            if (r.deinterleave && r.mfma_pipe == PIPE_FP6 && (fc.resamp || noise_shape) && !r.fine && C == Cin && (Cin == 8 || Cin == 4) &&
                !nocoop) {
                r.coop = true; r.deinterleave = false; r.B = 1;
            }
            // byte-interleaved stereo (DFF files, the CLI's default -f I) into frames through a pipelined kernel (fp6: M = 32, 64; int8: M = 8, 16):
            // the same, inside one wave
            // (the scratch flavours too: stereo DFF input into the 48k cascade and the noise shaper; not the two passes of 32-bit taps)
            if (r.deinterleave && ((r.mfma_pipe == PIPE_FP6 || (r.mfma_pipe == PIPE_INT8 && M < 64)) && !r.fine) && Cin == 2 && C == 2 &&
                !nocoop) {
                r.il2 = true; r.deinterleave = false; r.B = 1;
            }
        }
        if (r.fine && r.mfma_v2) {
            // the residual table goes through the same builders; which pipelined kernel serves it is decided on ITS digits
            std::vector<int32_t> lo_half;
            const d2d_filter_def lo_def = residual_def(f, lo_half);
            r.mfma_pipe_lo = mfma2_pipelined(fir_args_static(p, fc, epi, r, &lo_def), M, N);
        }
    }
    if (!r.poly && r.kernel == D2D_KERNEL_MFMA && Cin == 1 && C == 1 && !r.fine && !noise_shape && !fc.resamp &&
        !(p.debug_flags & (D2D_DBG_NO_PIPE | D2D_DBG_MFMA_V1 | D2D_DBG_NO_MX))) {
        // would the stereo conversion of this format run a pipelined kernel?  Then so can a mono stream, two halves of a call at a time
        FirArgs a2 = fir_args_static(p, fc, epi, r);
        a2.epi.channels = 2; a2.in_channels = 2;
        const int p2 = mfma2_pipelined(a2, M, N);
        if (p2 == PIPE_FP6 || p2 == PIPE_INT8) r.mono2_pipe = p2;
    }
    r.table_variant = route_table_variant(r);
    return D2D_OK;
}

std::string route_kernel_name(const FirRoute& r, const FilterChoice& fc, const Epilogue& epi) {
    const int M = fc.fir->M, Mb = M / 8, N = fc.fir->ntaps;
    const bool noise_shape = epi.dither == 'N';
    auto num = [](long v) { return std::to_string(v); };
    const int dkind = epi.dither == 'T' ? 1 : epi.dither == 'R' ? 2 : 0;
    const bool scr = fc.resamp || noise_shape;           // the kernel writes integers to the scratch, not frames
    if (r.poly) {
        if (r.poly_plain) return "d2d_poly_plain_kernel";
        const bool intq = epi.gain == 1.0 && (epi.bits == 24 || epi.bits == 16) && epi.dither != 'F';
        const int kind = noise_shape ? 4 : !intq ? 3 : dkind;
        return "d2d_fir_px_kernel<" + num(fc.poly->Lp) + ", " + num(fc.poly->Mp) + ", " + num(fc.poly->NP) + ", " + num(px_groups(*fc.poly)) + ", " +
               num(kind) + ">";
    } else if (r.kernel != D2D_KERNEL_MFMA || !r.mfma_v2) {
        return (r.kernel == D2D_KERNEL_LUT ? "d2d_fir_lut_kernel<" : "d2d_fir_mfma_kernel<") + num(Mb) + ">";
    } else if (r.mfma_pipe == PIPE_FP6) {
        return "d2d_fir_mx_kernel<" + num(Mb) + ", " + num(N) + ", " + num(mx_groups(Mb)) + ", " +
               num(scr || epi.sample_bytes == 4 ? 0 : dkind) + ", " + num(scr ? 0u : epi.sample_bytes) + ">";
    } else if (r.mfma_pipe == PIPE_INT8) {
        return "d2d_fir_mfma3_kernel<" + num(Mb) + ", " + num(mfma2_pairs(M, N)) + ", 0, " + num(scr ? 0 : dkind) + ", " +
               num(scr ? 0u : epi.sample_bytes) + ">";
    }
    return "d2d_fir_mfma2_kernel<" + num(Mb) + ", " + num(mfma2_pairs(M, N)) + ", " + num(epi.channels == 1 ? 1 : 2) + ">";
}

// ---- the launch plans ------------------------------------------------------------------------------------------------------------
// One builder per kernel family.  Each chooses the instantiation from the arguments (the unit lists' comments say which ones an object holds),
// fills the kernel's argument struct and lays out the block's LDS.  A plan whose `unit` stays -1 is one no compiled kernel serves.

constexpr size_t LDS_BYTES = 160 * 1024;

static void instantiation(FirLaunch& l, int family, std::initializer_list<int> targs) {
    static const char* const KERNEL[] = {"d2d_fir_lut_kernel", "d2d_fir_mfma_kernel", "d2d_fir_mfma2_kernel", "d2d_fir_mfma3_kernel",
                                         "d2d_fir_mx_kernel", "d2d_fir_px_kernel", "d2d_poly_plain_kernel"};
    l.family = family;
    l.nt = 0;
    l.name = KERNEL[family];
    for (int v : targs) { l.name += (l.nt ? ", " : "<") + std::to_string(v); l.t[l.nt++] = v; }
    if (l.nt) l.name += ">";
}

// the requantiser's flavour of the pipelined kernels' frames: the dither kinds of the all-integer one (0 none, 1 triangular, 2 rectangular),
// + 4 with the f64 one (`gain`), whose 7 is float frames with the float dither
static int pipe_kind(const Mfma2Args& m, bool gain) {
    if (gain && m.f.epi.sample_bytes == 4) return m.f.epi.dither == 'F' ? 7 : 4;
    return (gain ? 4 : 0) + (m.f.epi.sample_bytes == 4 ? 0 : m.dkind == 1 ? 1 : m.dkind == 2 ? 2 : 0);
}

static FirLaunch lut_plan(const FirArgs& a, int MB) {
    FirLaunch l;
    instantiation(l, FIR_LUT, {MB});
    l.m.f = a;
    const int LS = MB >= 8 ? MB : 8;
    const size_t span = (size_t)((255 * LS + 8 * (a.nq + 1) + 16 + 15) & ~15);
    l.lds = (size_t)a.ntab * 128 + 4 * sizeof(double) + span;
    l.nwaves = LUT_THREADS / 64;
    l.tile = (uint32_t)(LUT_THREADS * (MB >= 8 ? 1 : 8 / MB));
    l.block_tiles = 1;
    l.rows_per_file = a.epi.channels;
    if (MB == 1 || MB == 2 || MB == 4 || MB == 8 || MB == 16) l.unit = MB;
    return l;
}

static FirLaunch mfma_plan(const FirArgs& a, const MfmaLayout& g) {
    FirLaunch l;
    const int MB = g.M / 8;
    instantiation(l, FIR_MFMA, {MB});
    mfma_geometry(a, g, l.m1, l.lds);
    l.nwaves = l.block_tiles = l.m1.nwaves;
    l.tile = 256;
    l.rows_per_file = l.m1.ngroups;       // one row per (file, channel group)
    if (mfma_supported(g.M, g.N) && l.lds <= LDS_BYTES) l.unit = MB;
    return l;
}

// the fp6 kernel: `l.m` holds the two-group geometry's arguments; the LDS layout is the kernel's own
static void mx_plan(FirLaunch& l, int MB, int NT) {
    Mfma2Args& m = l.m;
    const FirArgs& a = m.f;
    m.npairs = mx_pairs(a, MB, NT);
    // M = 128 has no other kernel whose conditions gainq would have to respect: every frame format that is not the all-integer requantiser's
    if (MB == 16 && m.npairs == 1) m.gainq = (!a.to_scratch && (a.epi.gain != 1.0 || m.qsh != 0 || (a.epi.bits == 32 && a.epi.dither == 'F'))) ? 1u : 0u;
    const MxFlavour fl = a.taps32 ? MX_WIDE : m.npairs == 1 && m.gainq && !a.to_scratch ? MX_GAIN : MX_INT;
    const int NPR = a.taps32 ? 1 : (int)m.npairs, ND = fl == MX_WIDE ? 7 : 5, PH = ND == 7 ? 4 : 6, G = mx_g(MB);
    // the exact integers for the scratch only where a wave converts one pair at unit gain
    const bool scr = a.to_scratch && fl == MX_INT && NPR == 1;
    const int KIND = scr ? 0 : pipe_kind(m, fl != MX_INT), SBY = scr ? 0 : (int)a.epi.sample_bytes;
    instantiation(l, FIR_MX, {MB, NT, G, KIND, SBY, NPR, ND});     // (all seven arguments: the way rocprofv3 prints the instantiation)
    l.tile = 32u * (uint32_t)PH * (uint32_t)G;
    // LDS: the shared tap table, then per wave two stream buffers and the output slice; eight waves per block = two per SIMD
    m.off_waves = mx_nres_of(MB, NT, SBY, NPR, ND) == mx_nf(MB, NT, PH) ? 0u : (uint32_t)mx_nf(MB, NT, PH) * MX_FRAG_BYTES;    // (no table where every fragment is resident)
    m.off_out = 2u * (uint32_t)mx_stream_bytes(MB, NT, G, PH);
    m.wave_lds = m.off_out + 2u * (uint32_t)NPR * l.tile * 4u;   // the slice: a row of `tile` dwords per channel (the scratch flavour too: its integers leave as rows of the slice)
    uint32_t nwaves = waves_asked(a, D2D_MX_THREADS / 64);
    while (nwaves > 1 && (size_t)m.off_waves + (size_t)nwaves * m.wave_lds > LDS_BYTES) { if (NPR > 1) --nwaves; else nwaves >>= 1; }
    const bool coop = SBY == 0 && a.coop;                   // a block = all channel pairs of a file on one tile: one wave per pair, one grid row per file
    if (coop) nwaves = a.epi.channels / 2u;
    m.nwaves = l.nwaves = nwaves;
    l.block_tiles = coop ? 1u : nwaves;
    if (coop || NPR > 1) l.rows_per_file = 1;               // (several pairs per wave: whole frames from one wave)
    l.lds = (size_t)m.off_waves + (size_t)nwaves * m.wave_lds;
    l.unit = l.lds <= LDS_BYTES ? mx_find(MB, NT, fl, NPR) : -1;
}

// the pipelined int8 kernel, on the two-group geometry's arguments likewise
static void m3_plan(FirLaunch& l, int MB, int NPG, int NT) {
    Mfma2Args& m = l.m;
    const FirArgs& a = m.f;
    const bool scr = a.to_scratch != 0;
    const int KIND = scr ? 0 : pipe_kind(m, m.gainq != 0), SBY = scr ? 0 : a.epi.sample_bytes == 4 ? 4 : a.epi.sample_bytes == 3 ? 3 : 2;
    instantiation(l, FIR_M3, {MB, NPG, 0, KIND, SBY});
    l.tile = M2_TILE;
    // LDS: the shared tap table, then two stream buffers per wave; eight waves per block = two per SIMD
    m.off_waves = (uint32_t)(2 * NPG) * 1024u;
    m.wave_lds = 2u * (uint32_t)m2_stream_bytes(MB, NPG);
    m.off_out = m.wave_lds;
    if (D2D_M3_STAGED && MB == 1 && SBY != 0) m.wave_lds += (uint32_t)M2_TILE * 2u * (uint32_t)SBY;     // the tile's frames, staged for whole-line stores
    m.nwaves = waves_asked(a, 8);
    while (m.nwaves > 1 && (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds > LDS_BYTES) m.nwaves >>= 1;
    l.nwaves = l.block_tiles = m.nwaves;
    l.lds = (size_t)m.off_waves + (size_t)m.nwaves * m.wave_lds;
    // every unit holds the scratch flavour; frames where its row names the tap count, their gain flavours for M = 8 and 16
    const int u = m3_find(MB, NPG);
    if (l.lds <= LDS_BYTES && (scr || (m3_frames(u, NT) && (KIND < 4 || MB < 4)))) l.unit = u;
}

// a shape of the two-group geometry: the two-group kernel itself or the pipelined kernel the engine built its table for (FirArgs::pipelined)
static FirLaunch mfma2_plan(const FirArgs& a, int M, int N) {
    FirLaunch l;
    const int MB = M / 8, NPG = mfma2_pairs(M, N);
    mfma2_geometry(a, MB, NPG, l.m, l.lds);
    l.rows_per_file = l.m.ngroups;        // one row per (file, channel group)
    if (a.pipelined == PIPE_FP6) { mx_plan(l, MB, N); return l; }      // (M = 128 has no two-group kernel at all)
    const bool fits = l.lds <= LDS_BYTES;
    if (a.pipelined) {
        m3_plan(l, MB, NPG, N);
    } else {
        // the epilogue flavour: the integers for the stage-A scratch, stereo 24-bit packed in registers, or anything via LDS
        instantiation(l, FIR_MFMA2, {MB, NPG, a.epi.channels == 1 ? 1 : 2, mfma2_epilogue(a, l.m)});
        l.nwaves = l.block_tiles = l.m.nwaves;
        l.tile = M2_TILE;
        int row = 0;
#define X(mb, npg) if (MB == mb && NPG == npg) l.unit = row; ++row;
        D2D_M2_SHAPES(X)
#undef X
    }
    if (!fits) l.unit = -1;
    return l;
}

static FirLaunch px_plan(const d2d_params& p, const d2d_poly_def& pd, const Epilogue& epi, const FirRoute& r) {
    FirLaunch l;
    PxArgs& a = l.px;
    a.in_channels = p.channels; a.B = r.B; a.keep = r.keep; a.msb = p.endianness == D2D_MSB_FIRST ? 1u : 0u;
    a.to_scratch = epi.dither == 'N' ? 1u : 0u;
    a.il2 = r.il2 ? 1u : 0u;
    a.epi = epi;
    a.Lp = (uint32_t)pd.Lp; a.Mp = (uint32_t)pd.Mp; a.NP = (uint32_t)pd.NP; a.D = pd.D; a.S = pd.S;
    const uint32_t C = epi.channels;
    if (r.poly_plain) {
        instantiation(l, FIR_PX_PLAIN, {});
        // bytes a tile's windows span: 255 outputs further on, the window itself, up to 15 bytes in front, 16 of slack
        l.px_span = (uint32_t)((((uint64_t)(PXP_THREADS - 1) * pd.Mp / pd.Lp + pd.NP + 7) / 8 + 15 + 16 + 15) & ~(uint64_t)15);
        l.lds = (((size_t)pd.Lp * pd.NP * 4 + 15) & ~(size_t)15) + 32 + l.px_span;
        l.nwaves = PXP_THREADS / 64;
        l.tile = PXP_THREADS;
        l.block_tiles = 1;
        l.rows_per_file = C;
        l.unit = 0;
        return l;
    }
    a.dkind = epi.dither == 'T' ? 1u : (epi.dither == 'R' ? 2u : 0u);
    a.fbits = pd.S - ((int)epi.bits - 1);
    a.qmin_i = epi.bits == 32 ? 0 : -(1 << (epi.bits - 1));
    a.qmax_i = epi.bits == 32 ? 0 : (1 << (epi.bits - 1)) - 1;
    a.qsh = epi.bits == 20 ? 4u : 0u;
    // KIND: the integers for the noise shaper (4), the f64 requantiser (3), or the all-integer one's dither kind
    const bool intq = epi.gain == 1.0 && (epi.bits == 24 || epi.bits == 16) && epi.dither != 'F';
    const int LP = pd.Lp, MP = pd.Mp, NP = pd.NP, G = px_groups(pd);
    instantiation(l, FIR_PX, {LP, MP, NP, G, a.to_scratch ? 4 : !intq ? 3 : (int)a.dkind});
    if (G == 0) return l;                 // (no row for the table)
    l.tile = 160u * (uint32_t)G;
    a.cw = C == 1 ? 1u : 2u;
    a.ngroups = (C + a.cw - 1) / a.cw;
    a.off_waves = (uint32_t)px_nslot(LP, MP, NP, G) * PX_FRAG_BYTES;
    a.off_out = a.cw * (uint32_t)px_stream_bytes(LP, MP, NP, G);
    a.wave_lds = a.off_out + a.cw * l.tile * 4u + 256u;                // (+ 64 dwords nobody reads: where the pipelined epilogue puts half 1's third slot)
    a.nwaves = PX_THREADS / 64;
    while (a.nwaves > 1 && (size_t)a.off_waves + (size_t)a.nwaves * a.wave_lds > LDS_BYTES) --a.nwaves;
    l.nwaves = l.block_tiles = a.nwaves;
    l.rows_per_file = a.ngroups;
    l.lds = (size_t)a.off_waves + (size_t)a.nwaves * a.wave_lds;
    if (l.lds <= LDS_BYTES) l.unit = px_find(pd);
    return l;
}

FirLaunch fir_launch(const d2d_params& p, const FilterChoice& fc, const Epilogue& epi, const FirRoute& r, FirPass pass, const d2d_filter_def* lo) {
    if (r.poly) return px_plan(p, *fc.poly, epi, r);
    const int M = fc.fir->M, N = fc.fir->ntaps;
    FirArgs a = fir_args_static(p, fc, epi, r, pass == PASS_LO ? lo : nullptr);
    if (pass == PASS_MONO2) {
        a.epi.channels = 2; a.in_channels = 2;
        a.B = 0x40000000u;     // (one "block" per half: the gather path's layout rule then reads half c at c * half)
        a.pipelined = (uint32_t)r.mono2_pipe; a.mono2 = 1;
        return mfma2_plan(a, M, N);
    }
    if (r.kernel == D2D_KERNEL_LUT) return lut_plan(a, M / 8);
    return r.mfma_v2 ? mfma2_plan(a, M, N) : mfma_plan(a, mfma_layout(M, N));
}

}  // namespace d2d
