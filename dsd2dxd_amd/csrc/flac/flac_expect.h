// flac_expect.h -- the cooperative verifier's rule: when a frame may be called good WITHOUT decoding its codes one after the other.
// Plain C++, as flac_parse.h and flac_lpc.h: g++ for the host twin (d2d_flac_host.cpp: d2d_flac_verify_host_method), hipcc for the
// kernel (d2d_flac_verify.hip: flac_verify_coop_kernel).  It restates no rule of flac_parse.h: the header, the CRCs, the field readers,
// the PCM unpacking and the coded signals are that header's, called from here.
//
// THE IDEA.  A frame's codes are serial only for a reader that does not know the samples.  The verifier holds the PCM, so it can
// compute every residual under the predictor the subframe header names, hence every code and every code's length, hence every bit
// position, and then COMPARE the frame's bits with the bits it expects -- all samples at once.  What stays serial is short: the frame
// header, per subframe its head, and per Rice partition one 5-bit parameter, which sits where the lengths of the partition before it end.
//
// THE ACCEPTANCE RULE.  The fast path only ever says "this frame is good".  It accepts a frame exactly when
//   E1. rules 2 to 5 of flac_parse.h hold (rule 1, the size, is the caller's, in front of either path): parse_header gives no reason,
//       the header and two more bytes fit the frame, the CRC-16 over all bytes in front of the last two is the one stored there;
//   E2. every subframe is verbatim, fixed 0 .. 4 or LPC, without wasted bits, with an order of at most n, LPC precision below 16 and a
//       shift below 16, Rice method `01`, a partition order p <= MAX_PORDER with n % 2^p == 0 and (n >> p) >= order, and no partition
//       parameter 31 (walk_subframe; the parameter where the partitions are walked);
//   E3. every residual x(i) - prediction, the prediction computed from the ORIGINAL samples by predict_fixed / predict_lpc in 64 bits,
//       zigzags into 32 bits (what the encoders write is far below; a frame beyond it is not handled here);
//   E4. no running position passes the frame's last body bit, 8 * (size - 2): decided from lengths, before a bit there is read;
//   E5. every compared field equals what is expected: the verbatim and warm-up samples in `bps` bits, every Rice code -- u >> k zeros,
//       a one, the k low bits of u (code_matches);
//   E6. the bits behind the last subframe up to the byte boundary are zero, and that boundary is two bytes in front of the frame's end.
// Everything else -- a mismatch, a field outside E2, a position that would pass the end, a frame E3 does not handle -- is handed to
// d2dparse::verify_frame, the serial parser, whose answer is the block's reason.  Reasons, their order and the agreement of host and
// device therefore stay defined in flac_parse.h alone.  Every bit of an accepted frame was parsed (E1, E2), compared (E5) or checked
// as padding or CRC (E1, E6) exactly once.
//
// WHY ACCEPT MEANS D2D_FLAC_BAD_NONE, AND THE REVERSE.
//   =>  Let the bits equal the canonical serialisation of (the parsed parameters P, the PCM).  The serial parser reads the same P (the
//       same fields through the same readers).  By induction over i it has decoded x(0 .. i-1) = the original, so its prediction is the
//       one computed here from the original; the code at the position computed here is the code of u(i) under k, so it reads u(i), adds
//       the prediction and gets x(i), which fits its sample size because the original does.  Its position behind the code is the one
//       computed here.  Rules 6 to 8 pass; rules 2 to 5 and 7 are E1 and E6.
//   <=  Let the serial parser decode the frame to the PCM under parameters P.  The residuals are determined by P and the PCM, a Rice
//       code is determined by its residual and k, so the bits are the expected ones; a frame of the repertoire E2 / E3 is then accepted
//       here, and one outside it reaches the serial parser itself.
// So the record of a call does not depend on the method; only the count of blocks each path decided (d2d_flac_verify_stats) does.
//
// MEMORY SAFETY.  No address depends on frame contents other than through range-checked fields: positions come from the size (rule 1,
// checked first) and from lengths computed from the PCM, and a position beyond the body is a reject (E4) decided before the read.
#pragma once
#include "flac_parse.h"

namespace d2dexpect {

constexpr uint32_t MAX_PORDER = 6;             // 64 partitions: what the encoders' search reaches (flac_lpc.h: search_pmax)
constexpr uint32_t FALLBACK_BIT = 0x80000000u; // of a block's status word: the serial parser decided it (status_word keeps bits 0 .. 20)

// `len` (0 .. 32) bits at bit `pos` of a frame image, most significant first.  Img has word(w): bytes 4w .. 4w+3 of the frame, big-endian.
// The caller has checked pos + len against the frame; word w + 1 is touched only where the field reaches it.
template <class Img>
D2D_PARSE_HD uint32_t peek(const Img& img, uint32_t pos, uint32_t len) {
    if (len == 0) return 0;
    const uint32_t w = pos >> 5, o = pos & 31;
    const uint64_t two = ((uint64_t)img.word(w) << 32) | (o + len > 32 ? img.word(w + 1) : 0u);
    return (uint32_t)((two << o) >> (64 - len));
}
// the image of a frame in host memory: never a byte outside [p, p + size)
struct ByteImage {
    const uint8_t* p;
    uint32_t size;
    D2D_PARSE_HD uint32_t word(uint32_t w) const {
        uint32_t v = 0;
        for (uint32_t i = 0; i < 4; ++i) v = (v << 8) | (4 * w + i < size ? p[4 * w + i] : 0u);
        return v;
    }
};
// flac_parse.h's field readers (read, sread, bad) over an image, from any bit: the walk below runs on this or on d2dparse::BitReader
template <class Img>
struct ImageReader {
    const Img& img;
    uint32_t pos, end;                         // bits
    bool bad = false;
    D2D_PARSE_HD ImageReader(const Img& i, uint32_t p, uint32_t e) : img(i), pos(p < e ? p : e), end(e) {}
    D2D_PARSE_HD uint32_t read(uint32_t n) {
        if (n == 0) return 0;
        if (bad || n > end - pos) { bad = true; pos = end; return 0; }
        const uint32_t v = peek(img, pos, n);
        pos += n;
        return v;
    }
    D2D_PARSE_HD int32_t sread(uint32_t n) {
        const uint32_t v = read(n);
        return n >= 32 ? (int32_t)v : (int32_t)(v ^ (1u << (n - 1))) - (int32_t)(1u << (n - 1));
    }
};

// What the head of a subframe says (E2).  `bits`: from the subframe's first bit to the first partition's parameter -- the head, the
// warm-up samples, the LPC fields, method and partition order; for a verbatim subframe the 8 bits of the head.
struct SubHead {
    bool verbatim, lpc;
    uint32_t order, precision, shift, porder, bits;
};
// E2 on the subframe the reader stands at; the warm-up samples are stepped over (the caller compares them), the LPC coefficients go to
// coef[0 .. order).  False: not of the repertoire, or the bits ran out.
template <class Reader>
D2D_PARSE_HD bool walk_subframe(Reader& br, uint32_t n, uint32_t bps, SubHead& h, int32_t* coef) {
    const uint32_t head = br.read(8);
    if (br.bad || (head & 0x81u)) return false;                     // the first bit; wasted bits
    const uint32_t type = head >> 1;
    h.verbatim = type == 1; h.lpc = type >= 32; h.order = 0; h.precision = 0; h.shift = 0; h.porder = 0; h.bits = 8;
    if (h.verbatim) return true;
    if (h.lpc) h.order = type - 31;
    else if (type >= 8 && type <= 12) h.order = type - 8;
    else return false;                                              // constant, reserved
    if (h.order > n) return false;
    for (uint32_t i = 0; i < h.order; ++i) (void)br.read(bps);
    if (h.lpc) {
        h.precision = br.read(4) + 1;
        h.shift = br.read(5);
        if (br.bad || h.precision == 16 || h.shift >= 16) return false;
        for (uint32_t j = 0; j < h.order; ++j) coef[j] = br.sread(h.precision);
    }
    const uint32_t method = br.read(2);
    h.porder = br.read(4);
    if (br.bad || method != 1 || h.porder > MAX_PORDER) return false;
    if ((n & ((1u << h.porder) - 1)) || (n >> h.porder) < h.order) return false;
    h.bits = 8 + h.order * bps + (h.lpc ? 9 + h.order * h.precision : 0) + 6;
    return true;
}

// sample i of the coded signal the subframe `sig.begin` chose (rule 9 of flac_parse.h), from the block's PCM
D2D_PARSE_HD int32_t coded_sample(const d2dparse::VerifySig& sig, uint32_t i) {
    if (sig.kind == 0) return d2dparse::pcm_sample(sig.pcm, (size_t)i * sig.channels + sig.c, sig.depth);
    const int32_t l = d2dparse::pcm_sample(sig.pcm, (size_t)i * 2, sig.depth), r = d2dparse::pcm_sample(sig.pcm, (size_t)i * 2 + 1, sig.depth);
    return sig.kind == 1 ? (l + r) >> 1 : l - r;
}
// the predictions of rule 6: x1 .. x4 are x(i - 1) .. x(i - 4)
D2D_PARSE_HD int64_t predict_fixed(uint32_t order, int64_t x1, int64_t x2, int64_t x3, int64_t x4) {
    return order == 0 ? 0 : order == 1 ? x1 : order == 2 ? 2 * x1 - x2 : order == 3 ? 3 * x1 - 3 * x2 + x3 : 4 * x1 - 6 * x2 + 4 * x3 - x4;
}
// ... x points at x(i): x[-1 - m] is x(i - 1 - m)
D2D_PARSE_HD int64_t predict_lpc(const int32_t* x, const int32_t* coef, uint32_t order, uint32_t shift) {
    int64_t sum = 0;
    for (uint32_t m = 0; m < order; ++m) sum += (int64_t)coef[m] * x[-1 - (int32_t)m];
    return sum >> shift;
}
D2D_PARSE_HD int64_t predict(const SubHead& h, const int32_t* x, const int32_t* coef) {
    if (h.lpc) return predict_lpc(x, coef, h.order, h.shift);
    return predict_fixed(h.order, h.order > 0 ? x[-1] : 0, h.order > 1 ? x[-2] : 0, h.order > 2 ? x[-3] : 0, h.order > 3 ? x[-4] : 0);
}
// the unsigned value whose Rice code carries residual r: the inverse of the parser's r = (u >> 1) ^ -(u & 1)
D2D_PARSE_HD uint64_t zigzag(int64_t r) { return ((uint64_t)r << 1) ^ (uint64_t)(r >> 63); }
// a code's bits under parameter k (below 31)
D2D_PARSE_HD uint64_t code_len(uint32_t u, uint32_t k) { return (uint64_t)(u >> k) + 1 + k; }
// the samples of partition j: [first, stop)
D2D_PARSE_HD uint32_t partition_first(uint32_t j, uint32_t psz, uint32_t order) { return j ? j * psz : order; }
// E5 for one code at `pos`; the caller has checked pos + code_len(u, k) against the body
template <class Img>
D2D_PARSE_HD bool code_matches(const Img& img, uint32_t pos, uint32_t u, uint32_t k) {
    for (uint32_t left = u >> k; left;) {
        const uint32_t c = left < 32 ? left : 32;
        if (peek(img, pos, c)) return false;
        pos += c; left -= c;
    }
    return peek(img, pos, k + 1) == ((1u << k) | (u & ((1u << k) - 1)));
}
// E5 for a verbatim or warm-up sample in `bps` bits
template <class Img>
D2D_PARSE_HD bool sample_matches(const Img& img, uint32_t pos, int32_t x, uint32_t bps) {
    return peek(img, pos, bps) == ((uint32_t)x & (0xFFFFFFFFu >> (32 - bps)));
}
// E6 at the bit behind the last subframe
template <class Img>
D2D_PARSE_HD bool tail_ok(const Img& img, uint32_t pos, uint32_t body_end) {
    const uint32_t pad = (8 - pos % 8) % 8;
    return pos + pad == body_end && peek(img, pos, pad) == 0;
}

// The rule on one frame, sample after sample: the host twin of flac_verify_coop_kernel, which takes the same decisions from the same
// functions with the samples spread over a workgroup.  `x` lends room for one coded signal, n words.
inline bool accept_frame(const uint8_t* frame, uint32_t size, const d2dparse::Expect& ex, const uint8_t* pcm, const uint16_t* crc_tab, int32_t* x) {
    d2dparse::Header h;
    if (d2dparse::parse_header(frame, size, ex, h) || size < h.bytes + 2) return false;
    if (d2dparse::crc16(frame, size - 2, crc_tab) != (((uint32_t)frame[size - 2] << 8) | frame[size - 1])) return false;
    const ByteImage img{frame, size};
    const uint32_t body_end = 8 * (size - 2), n = h.n, channels = h.assignment < 8 ? h.assignment + 1 : 2;
    d2dparse::VerifySig sig{pcm, ex.channels, ex.depth, 1, nullptr};
    int32_t coef[d2dparse::MAX_LPC_ORDER];
    uint64_t pos = 8 * h.bytes;                                     // 64 bits: a sum may pass the end by far before it is looked at
    for (uint32_t s = 0; s < channels; ++s) {
        sig.begin(s, h.assignment);
        const uint32_t bps = ex.depth + (sig.kind == 2 ? 1 : 0);
        d2dparse::BitReader br(frame, (uint32_t)pos / 8, size - 2);
        (void)br.read((uint32_t)pos % 8);
        SubHead sh;
        if (!walk_subframe(br, n, bps, sh, coef)) return false;
        for (uint32_t i = 0; i < n; ++i) x[i] = coded_sample(sig, i);
        const uint32_t plain = sh.verbatim ? n : sh.order;           // the samples that stand as they are, behind the head
        if (pos + 8 + (uint64_t)plain * bps > body_end) return false;
        for (uint32_t i = 0; i < plain; ++i) if (!sample_matches(img, (uint32_t)pos + 8 + i * bps, x[i], bps)) return false;
        pos += sh.verbatim ? 8 + (uint64_t)n * bps : sh.bits;
        if (sh.verbatim) continue;
        const uint32_t psz = n >> sh.porder;
        for (uint32_t j = 0; j < (1u << sh.porder); ++j) {
            if (pos + 5 > body_end) return false;
            const uint32_t k = peek(img, (uint32_t)pos, 5);
            if (k == 31) return false;
            pos += 5;
            for (uint32_t i = partition_first(j, psz, sh.order); i < (j + 1) * psz; ++i) {
                const uint64_t u = zigzag((int64_t)x[i] - predict(sh, x + i, coef));
                if (u >> 32) return false;
                if (pos + code_len((uint32_t)u, k) > body_end) return false;
                if (!code_matches(img, (uint32_t)pos, (uint32_t)u, k)) return false;
                pos += code_len((uint32_t)u, k);
            }
        }
    }
    return tail_ok(img, (uint32_t)pos, body_end);
}

}  // namespace d2dexpect
