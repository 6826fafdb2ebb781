// flac_frame_enc.h -- the host FLAC frame encoder: the one copy that FlacSink (host/pcm_sink.cpp) and
// d2d_flac_encode_host (flac/d2d_flac_host.cpp) both run, and the byte-for-byte definition of what the GPU
// kernels of flac/d2d_flac.hip produce.  Host code only (no HIP).  The rules' small arithmetic -- rice_k, zigzag,
// search_pmax, the header bit counts, the LPC routine -- is flac_lpc.h, the one copy the kernels compile as well.  Every
// subframe, effort 0's too, is a Plan written by put_subframe.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "flac_lpc.h"

namespace d2dhost {

using namespace d2drice;       // rice_k, zigzag, search_pmax and the header bit counts: the copy the GPU kernels compile too

// Integer depths only.  Frames are independent of each other, so a batch of them is encoded on as many threads and written in
// order.  (The reference uses the flac-codec crate, Cargo.lock:299-307.)  Three efforts, all with fixed block size:
//
// EFFORT 0: fixed-order-2 prediction, one Rice partition per subframe, independent channels (valid, modest compression).
//
// EFFORT 1: searched fixed predictors, partitioned Rice and stereo modes.  Every cost is an exact bit count and every tie has a
// fixed winner, so the host, the GPU and the Python restatement of the tests agree on every byte.  For a frame of n samples per
// channel, ch channels, depth d (header, CRCs and padding as at effort 0):
//   1. n < 16: the frame is the effort-0 frame.
//   2. Candidate signals: each channel at b = d bits; for ch == 2 also M = (L + R) >> 1 (arithmetic, floor) at b = d and
//      S = L - R at b = d + 1.
//   3. Residuals r_0 = x, r_o(i) = r_{o-1}(i) - r_{o-1}(i-1) for i >= o, o = 0 .. 4.  |x| <= 2^24 gives |r_4| <= 2^28: residuals
//      and u = zigzag(r) fit 32 bits, and no verbatim or escape-coded partition exists.
//   4. cost(o, p) = 8 + o b + 2 + 4 + sum over the 2^p partitions of (5 + sum of ((u >> k) + 1 + k)); partition j holds the
//      residuals with i in [j (n >> p), (j + 1)(n >> p)) and i >= o; its k is effort 0's rule on that partition: the smallest k
//      with 2^k >= floor(sum |r| / count), at most 30, written with the 5-bit method `01`.
//   5. Predictor order: the o in 0 .. 4 with the least cost(o, 0); the smallest o wins a tie.
//   6. Partition order: for that o, the p in 0 .. pmax with the least cost(o, p); the smallest p wins a tie.  pmax is the largest
//      p <= 6 with n % 2^p == 0 and (n >> p) >= 16.
//   7. ch == 2: the least of L + R (nibble 0001: L, R), L + S (1000: L, S), S + R (1001: S, R), M + S (1010: M, S); ties go to the
//      earlier one.  The sample-size code stays d's; the side subframe has d + 1-bit warm-up samples.  Other counts: independent.
//   8. Subframe: 0, 001ooo, 0; o warm-up samples of b bits; 01, pppp; per partition kkkkk and its codes.
// (o = 2, p = 0) and the independent assignment are always candidates and the costs are exact, so an effort-1 frame is never
// longer than the effort-0 frame of the same samples: THE BOUND of include/dsd2dxd_amd.h holds for both.
//
// EFFORT 12: effort 1, and per candidate signal linear predictors of order 4, 8 and 12 (the value is the highest order searched).
// The autocorrelation is exact integer arithmetic; what is floating point (rule 13) is one serial f64 routine, flac_lpc.h, compiled
// from one source for the host and the GPU.  For a frame of n samples per channel and each candidate signal x of b bits (rule 2):
//   9. n < 64: the frame is the effort-1 frame (below 16 samples the effort-0 frame).
//  10. The effort-1 plan: rules 3 to 6 on x give (o1, p1, cost1).
//  11. Window: w(i) = (i + 1)(n - i); s = the bit length of floor((n + 1) / 2) floor((n + 2) / 2), the window's maximum;
//      y(i) = (x(i) w(i)) >> s, a 64-bit product and an arithmetic shift, so |y| <= |x| <= 2^24.
//  12. Autocorrelation: R(l) = sum over i = l .. n-1 of y(i) y(i - l), l = 0 .. 12: exact in signed 64 bits (|R| <= 2^60), so the
//      order of summation does not matter.
//  13. From R to coefficients, in IEEE f64, one operation per operation written, no fused multiply-add.  R(0) == 0: no LPC
//      candidates.  err = (double)R(0); for m = 1 .. 12: acc = (double)R(m); for j = 1 .. m-1: acc = acc - a[j] (double)R(m - j);
//      k = acc / err; a'[j] = a[j] - k a[m - j] for j < m, a'[m] = k; err = err (1.0 - k k); the first time !(err > 0) (NaN too) the
//      recursion stops for good, and that m is not reached.  For each m in {4, 8, 12} reached: a candidate needs every |a[j]| < 2^13
//      (a lesser bound would make the shift negative; anything not finite ends here) and cmax = max |a[j]| > 0; e = the smallest
//      integer with cmax < 2^e; sh = min(15, 13 - e); error feedback from t = 0, for j = 1 .. m: t = t + a[j] 2^sh,
//      q[j] = clamp(floor(t + 0.5), -8192, 8191), t = t - q[j].  The candidate is dropped when sum |q[j]| > 62 * 2^sh; for those that
//      remain |prediction| <= 62 * 2^24 and every residual has |r| < 2^30: no per-sample range check exists.
//  14. Residuals: r(i) = x(i) - ((sum over j = 1 .. P of q[j] x(i - j)) >> sh) for i >= P; a 64-bit sum, an arithmetic shift.
//  15. cost_lpc(P, p) = 8 + P b + 4 + 5 + 14 P + 2 + 4 + the partition terms of rule 4 with o = P.
//  16. The LPC plan: the P with the least cost_lpc(P, 0), the smaller P at a tie; for it the partition order by rule 6: cost2.
//  17. The signal's plan is the LPC plan only if cost2 < cost1, else the effort-1 plan.  Both partition searches come first, so an
//      effort-12 frame is never longer than the effort-1 frame of the same samples: THE BOUND, the workspace and the slots stand.
//  18. Stereo: rule 7 on the four signals' final costs.
//  19. LPC subframe: 0, 1ppppp (P - 1), 0; P warm-up samples of b bits; 1101 (precision 14, less one); sh in 5 bits; P coefficients
//      of 14 bits, two's complement, q[1] first; then 01, pppp and the partitions as in rule 8.
struct FlacFrameEnc {
    std::vector<uint8_t> out;
    uint64_t bitacc = 0; int bitn = 0;
    // (the tables are function-local statics of class type: built once, by whichever thread asks first)
    struct Crc8Table { uint8_t t[256]; Crc8Table() { for (int i = 0; i < 256; ++i) { uint8_t c = (uint8_t)i; for (int k = 0; k < 8; ++k) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : (c << 1)); t[i] = c; } } };
    struct Crc16Table { uint16_t t[256]; Crc16Table() { for (int i = 0; i < 256; ++i) { uint16_t c = (uint16_t)(i << 8); for (int k = 0; k < 8; ++k) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : (c << 1)); t[i] = c; } } };
    static const uint8_t* crc8_table() { static const Crc8Table tab; return tab.t; }
    static const uint16_t* crc16_table() { static const Crc16Table tab; return tab.t; }
    static uint8_t crc8(const uint8_t* p, size_t n) { const uint8_t* t = crc8_table(); uint8_t c = 0; for (size_t i = 0; i < n; ++i) c = t[c ^ p[i]]; return c; }
    static uint16_t crc16(const uint8_t* p, size_t n) { const uint16_t* t = crc16_table(); uint16_t c = 0; for (size_t i = 0; i < n; ++i) c = (uint16_t)((c << 8) ^ t[(c >> 8) ^ p[i]]); return c; }
    void bits_put(uint64_t v, int n) {
        while (n > 0) {
            int take = n > 32 ? 32 : n;
            uint64_t part = (v >> (n - take)) & ((1ull << take) - 1);
            bitacc = (bitacc << take) | part; bitn += take; n -= take;
            while (bitn >= 8) { out.push_back((uint8_t)(bitacc >> (bitn - 8))); bitn -= 8; }
        }
    }
    void bits_flush() { if (bitn) { out.push_back((uint8_t)(bitacc << (8 - bitn))); bitn = 0; } bitacc = 0; }
    void put_utf8(uint32_t v) {
        if (v < 0x80) { bits_put(v, 8); return; }
        int n = v < 0x800 ? 1 : v < 0x10000 ? 2 : v < 0x200000 ? 3 : v < 0x4000000 ? 4 : 5;
        bits_put(((0xFF00 >> (n + 1)) & 0xFF) | (v >> (6 * n)), 8);
        for (int i = n - 1; i >= 0; --i) bits_put(0x80 | ((v >> (6 * i)) & 0x3F), 8);
    }
    // the frame header with its CRC-8; `assignment` is the channel-assignment nibble
    void begin_frame(uint32_t n, uint32_t assignment, uint32_t depth, uint32_t frame_no, uint32_t BS) {
        out.clear(); bitn = 0; bitacc = 0;
        bits_put(0xFFF8, 16);                                          // sync, fixed block size
        bits_put(n == BS ? 0xC : 0x7, 4);                              // 4096, or 16-bit (n-1) at the end of the header
        bits_put(0x0, 4);                                              // sample rate from STREAMINFO
        bits_put(assignment, 4);
        bits_put(depth == 16 ? 4 : depth == 20 ? 5 : 6, 3); bits_put(0, 1);
        put_utf8(frame_no);
        if (n != BS) bits_put(n - 1, 16);
        bits_flush();
        out.push_back(crc8(out.data(), out.size()));
    }
    // zero bits to the next byte, then the CRC-16 of the frame
    void end_frame() {
        bits_flush();
        uint16_t c16 = crc16(out.data(), out.size());
        out.push_back((uint8_t)(c16 >> 8)); out.push_back((uint8_t)c16);
    }

    // ---- effort 1: the search (see the head of this file) --------------------------------------------------------------------
    // cost(o, p) of a signal of b bits whose order-o residuals are r[o .. n); ks (may be null) receives the 2^p parameters
    static uint32_t search_cost(const int32_t* r, uint32_t n, uint32_t o, uint32_t p, uint32_t b, uint8_t* ks) {
        uint32_t cost = fixed_header_bits(o, b);
        const uint32_t psz = n >> p;
        for (uint32_t j = 0; j < (1u << p); ++j) {
            const uint32_t lo = j * psz > o ? j * psz : o, hi = (j + 1) * psz;
            uint64_t sum = 0;
            for (uint32_t i = lo; i < hi; ++i) sum += (uint64_t)(r[i] < 0 ? -(int64_t)r[i] : (int64_t)r[i]);
            const uint32_t k = rice_k(sum, hi - lo);
            cost += PARAM_BITS;
            for (uint32_t i = lo; i < hi; ++i) cost += (zigzag(r[i]) >> k) + 1 + k;
            if (ks) ks[j] = (uint8_t)k;
        }
        return cost;
    }
    struct Plan {                               // what the search chose for one candidate signal
        uint32_t order = 0, porder = 0, bits = 0, cost = 0;
        bool lpc = false, verbatim = false;     // effort 12: `order` is an LPC order, with these coefficients; a frame of one or two samples, all warm-up
        int32_t q[d2dlpc::MAX_ORDER] = {}, shift = 0;
        uint8_t k[64];
        std::vector<int32_t> x, r;              // the signal, and its residuals at `order` (valid from index `order`)
    };
    Plan plans[4];
    std::vector<int32_t> rs[5];
    void search(Plan& pl, uint32_t n, uint32_t b) {
        pl.bits = b; pl.lpc = false; pl.verbatim = false;
        rs[0] = pl.x;
        for (uint32_t o = 1; o <= 4; ++o) {
            rs[o].resize(n);
            for (uint32_t i = o; i < n; ++i) rs[o][i] = rs[o - 1][i] - rs[o - 1][i - 1];
        }
        uint32_t best = 0, cost = 0;
        for (uint32_t o = 0; o <= 4; ++o) {                            // the smallest order wins a tie
            const uint32_t c = search_cost(rs[o].data(), n, o, 0, b, nullptr);
            if (o == 0 || c < cost) { best = o; cost = c; }
        }
        pl.order = best; pl.r = rs[best]; pl.porder = 0;
        const uint32_t pmax = search_pmax(n);
        for (uint32_t p = 1; p <= pmax; ++p) {                         // the smallest partition order wins a tie
            const uint32_t c = search_cost(pl.r.data(), n, best, p, b, nullptr);
            if (c < cost) { pl.porder = p; cost = c; }
        }
        pl.cost = search_cost(pl.r.data(), n, best, pl.porder, b, pl.k);
    }
    // ---- effort 12: rules 11 to 17 for one signal whose effort-1 plan `pl` holds ------------------------------------------------
    std::vector<int32_t> win, lres[d2dlpc::CANDIDATES];
    void search_lpc(Plan& pl, uint32_t n, uint32_t b) {
        using namespace d2dlpc;
        const uint32_t s = lpc_window_shift(n);
        win.resize(n);
        for (uint32_t i = 0; i < n; ++i) win[i] = lpc_window(pl.x[i], i, n, s);
        int64_t R[MAX_ORDER + 1];
        for (uint32_t l = 0; l <= (uint32_t)MAX_ORDER; ++l) {
            int64_t sum = 0;
            for (uint32_t i = l; i < n; ++i) sum += (int64_t)win[i] * win[i - l];
            R[l] = sum;
        }
        LpcCoefs co;
        lpc_coefficients(R, co);
        int best = -1; uint32_t cost = 0;
        for (int c = 0; c < CANDIDATES; ++c) {                         // the smaller order wins a tie
            if (!(co.valid >> c & 1u)) continue;
            const uint32_t P = 4 * (c + 1);
            std::vector<int32_t>& r = lres[c];
            r.resize(n);
            int32_t before[MAX_ORDER];
            for (uint32_t i = P; i < n; ++i) {
                for (uint32_t j = 0; j < P; ++j) before[j] = pl.x[i - 1 - j];
                r[i] = P == 4 ? lpc_residual<4>(pl.x[i], before, co.q[c], co.shift[c]) : P == 8 ? lpc_residual<8>(pl.x[i], before, co.q[c], co.shift[c])
                                                                                         : lpc_residual<12>(pl.x[i], before, co.q[c], co.shift[c]);
            }
            const uint32_t cc = lpc_coef_bits(P) + search_cost(r.data(), n, P, 0, b, nullptr);
            if (best < 0 || cc < cost) { best = c; cost = cc; }
        }
        if (best < 0) return;
        const uint32_t P = 4 * (best + 1), pmax = search_pmax(n);
        uint32_t porder = 0;
        for (uint32_t p = 1; p <= pmax; ++p) {                         // the smallest partition order wins a tie
            const uint32_t cc = lpc_coef_bits(P) + search_cost(lres[best].data(), n, P, p, b, nullptr);
            if (cc < cost) { porder = p; cost = cc; }
        }
        if (!(cost < pl.cost)) return;                                 // rule 17: the effort-1 plan stays unless LPC is strictly cheaper
        pl.lpc = true; pl.order = P; pl.porder = porder; pl.shift = co.shift[best];
        for (uint32_t j = 0; j < P; ++j) pl.q[j] = co.q[best][j];
        pl.r = lres[best];
        pl.cost = lpc_coef_bits(P) + search_cost(pl.r.data(), n, P, porder, b, pl.k);
    }
    void put_subframe(const Plan& pl, uint32_t n) {
        bits_put(0, 1); bits_put(pl.verbatim ? 1 : pl.lpc ? 32 + pl.order - 1 : 8 + pl.order, 6); bits_put(0, 1);
        for (uint32_t i = 0; i < pl.order; ++i) bits_put((uint64_t)(int64_t)pl.x[i] & ((1ull << pl.bits) - 1), (int)pl.bits);
        if (pl.verbatim) return;
        if (pl.lpc) {
            bits_put(d2dlpc::PRECISION - 1, 4); bits_put((uint64_t)pl.shift, 5);
            for (uint32_t j = 0; j < pl.order; ++j) bits_put((uint64_t)(int64_t)pl.q[j] & 0x3FFF, d2dlpc::PRECISION);
        }
        bits_put(1, 2); bits_put(pl.porder, 4);
        const uint32_t psz = n >> pl.porder;
        for (uint32_t j = 0; j < (1u << pl.porder); ++j) {
            const uint32_t k = pl.k[j];
            bits_put(k, 5);
            for (uint32_t i = j * psz > pl.order ? j * psz : pl.order; i < (j + 1) * psz; ++i) {
                const uint32_t u = zigzag(pl.r[i]);
                uint32_t q = u >> k;
                while (q >= 32) { bits_put(0, 32); q -= 32; }
                bits_put(1, (int)q + 1);
                if (k) bits_put(u & ((1u << k) - 1), (int)k);
            }
        }
    }
    void encode_search(const int32_t* buf, uint32_t n, uint32_t ch, uint32_t depth, uint32_t frame_no, uint32_t BS, bool lpc = false) {
        uint32_t first = 0, second = 1, nibble = ch - 1;
        if (ch == 2) {
            for (Plan& pl : plans) pl.x.resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                const int32_t l = buf[(size_t)i * 2], r = buf[(size_t)i * 2 + 1];
                plans[0].x[i] = l; plans[1].x[i] = r; plans[2].x[i] = (l + r) >> 1; plans[3].x[i] = l - r;
            }
            for (uint32_t s = 0; s < 4; ++s) {
                search(plans[s], n, s == 3 ? depth + 1 : depth);
                if (lpc) search_lpc(plans[s], n, s == 3 ? depth + 1 : depth);
            }
            const uint32_t L = plans[0].cost, R = plans[1].cost, M = plans[2].cost, S = plans[3].cost;
            uint32_t total = L + R;                                     // ties go to the earlier mode
            if (L + S < total) { total = L + S; first = 0; second = 3; nibble = 0x8; }
            if (S + R < total) { total = S + R; first = 3; second = 1; nibble = 0x9; }
            if (M + S < total) { total = M + S; first = 2; second = 3; nibble = 0xA; }
        }
        begin_frame(n, nibble, depth, frame_no, BS);
        if (ch == 2) { put_subframe(plans[first], n); put_subframe(plans[second], n); }
        else for (uint32_t c = 0; c < ch; ++c) {
            Plan& pl = plans[0];
            pl.x.resize(n);
            for (uint32_t i = 0; i < n; ++i) pl.x[i] = buf[(size_t)i * ch + c];
            search(pl, n, depth);
            if (lpc) search_lpc(pl, n, depth);
            put_subframe(pl, n);
        }
        end_frame();
    }

    // one frame of `n` interleaved samples starting at `buf`; effort 0 = fixed order 2, 1 = the search, 12 = the search with LPC
    void encode(const int32_t* buf, uint32_t n, uint32_t ch, uint32_t depth, uint32_t frame_no, uint32_t BS, uint32_t effort = 0) {
        if (effort != 0 && n >= 16) { encode_search(buf, n, ch, depth, frame_no, BS, effort == 12 && n >= d2dlpc::MIN_FRAME); return; }
        // effort 0's frame: independent channels, each the plan (order 2, partition order 0).  Both callers (FlacSink::write,
        // d2d_flac_encode_host_effort) sign-extend the samples from packed PCM of `depth` bits: |r| <= 2^25, no escape is needed.
        begin_frame(n, ch - 1, depth, frame_no, BS);
        Plan& pl = plans[0];
        pl.lpc = false; pl.verbatim = n <= 2; pl.order = pl.verbatim ? n : 2; pl.porder = 0; pl.bits = depth;
        pl.x.resize(n); pl.r.resize(n);
        for (uint32_t c = 0; c < ch; ++c) {
            uint64_t sum = 0;
            for (uint32_t i = 0; i < n; ++i) pl.x[i] = buf[(size_t)i * ch + c];
            for (uint32_t i = 2; i < n; ++i) {
                pl.r[i] = pl.x[i] - 2 * pl.x[i - 1] + pl.x[i - 2];
                sum += (uint64_t)(pl.r[i] < 0 ? -(int64_t)pl.r[i] : (int64_t)pl.r[i]);
            }
            pl.k[0] = (uint8_t)rice_k(sum, n > 2 ? n - 2 : 1);
            put_subframe(pl, n);
        }
        end_frame();
    }
};

}  // namespace d2dhost
