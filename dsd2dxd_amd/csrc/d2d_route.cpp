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
    const uint32_t wdbg = (a.dbg_flags >> 8) & 0xFFu;      // diagnostic override (d2d_params.debug_flags bits 8..15)
    m.nwaves = wdbg ? wdbg : 12u;
    if (m.nwaves < 1 || m.nwaves > 12) m.nwaves = 12;
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
    const bool frames_ok = !a.to_scratch && a.epi.channels == 2 && (a.epi.sample_bytes == 3 || a.epi.sample_bytes == 2) && m.qsh == 0 && !m.wide;
    const bool shape_ok = a.scale_bits >= 18 && a.scale_bits <= 30 && mfma3_supported(MB, NPG, NT);
    // ... or 32-bit float at 0 dB without the float dither: the sample is (float)v * 2^-S
    const bool noint = (a.dbg_flags & D2D_DBG_NO_INTQ) != 0;
    const bool float_ok = !noint && !a.to_scratch && a.epi.channels == 2 && a.epi.bits == 32 && a.epi.dither != 'F' && a.epi.gain == 1.0 && !m.wide &&
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

// the same conversions as mfma3_eligible, shape apart (the caller checks mx_supported and the engine mx_exact)
static bool mx_eligible(const FirArgs& a, const Mfma2Args& m, int MB, int N) {
    const bool range_ok = a.scale_bits >= 20 && a.scale_bits <= 30 && a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31) && a.mx_exact;
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
        const bool range_ok = a.scale_bits >= 20 && a.scale_bits <= 30 && a.sum_abs_q != 0 && a.sum_abs_q < (1ull << 31) && a.mx_exact;
        if (nomx || !mx_supported(MB, N) || !range_ok || noint16) return PIPE_NONE;
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
    // ... and stereo frames at another level than 0 dB (its gain flavours)
    if (!nomx && m.gainq && mx_gain_supported(MB, N) && a.mx_exact && a.scale_bits >= 20 && a.scale_bits <= 30 && (a.epi.bits == 32 || a.epi.sample_bytes == 2 || a.epi.sample_bytes == 3)) return PIPE_FP6;
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
    const uint32_t wdbg = (a.dbg_flags >> 8) & 0xFFu;      // diagnostic override (d2d_params.debug_flags bits 8..15)
    m.nwaves = wdbg ? wdbg : 12u;
    if (m.nwaves < 1 || m.nwaves > 12) m.nwaves = 12;
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

void mfma2_launch_args(const FirArgs& a, int MB, int NPG, int N, Mfma2Args& m, size_t& smem) {
    mfma2_geometry(a, MB, NPG, m, smem);
    if (a.pipelined != PIPE_FP6) return;                     // the fp6 kernel has its own LDS layout (and M = 128 no two-group one at all)
    m.npairs = mx_pairs(a, MB, N);
    if (m.npairs > 1u) return;                               // (one block row per file)
    if (MB == 16) m.gainq = (!a.to_scratch && (a.epi.gain != 1.0 || m.qsh != 0 || (a.epi.bits == 32 && a.epi.dither == 'F'))) ? 1u : 0u;
}

int mx_launch_unit(const Mfma2Args& m, int MB, int NT) {
    return m.f.taps32 ? mx_find(MB, NT, MX_WIDE, 1)
         : m.npairs > 1 ? mx_find(MB, NT, MX_INT, (int)m.npairs)
         : m.gainq && !m.f.to_scratch ? mx_find(MB, NT, MX_GAIN, 1)
         : mx_find(MB, NT, MX_INT, 1);
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

}  // namespace d2d
