// flac_parse.h -- the FLAC frame parser: the one copy that the host decoder and verifier (d2d_flac_host.cpp: d2d_flac_decode_host,
// d2d_flac_verify_host) and the GPU verify kernel (d2d_flac_verify.hip) both compile.  Plain C++, as flac_lpc.h: g++ for the host, hipcc
// for the device.  It reads what flac_frame_enc.h rules 8 and 19 can write, a little generalised, and gives every frame ONE reason
// (D2D_FLAC_BAD_*, include/dsd2dxd_amd.h).  No array here is indexed at run time: the history ring and the coefficients of an LPC
// subframe live in storage the caller hands in (the host's stack, the kernel's LDS), everything else is scalars.
//
// THE ORDER OF CHECKS.  A frame of `size` bytes is given with what the call expects of it: channels, depth, the block's n (0: any n up
// to 4096) and its frame number.  The first rule that fails names the reason; the later ones are not looked at.
//   1. SIZE (the callers, before the parser): the size-table entry is 0, above D2D_FLAC_FRAME_BOUND(4096), reaches beyond bytes_out,
//      or, for the last block, does not end at bytes_out.
//   2. HEADER: the 14-bit sync code and the reserved bit behind it; block-size code 0; sample-rate code 15; channel assignment above
//      10; sample-size code 3; the reserved bit; a frame number that is not UTF-8 of at most 6 bytes (7 with the variable-block-size
//      bit); a header that does not fit into the frame; then the fields against the call: n, channels (a stereo assignment has 2),
//      depth, and -- in a fixed-block-size frame -- the frame number.
//   3. CRC8 over the header bytes.
//   4. UNSUPPORTED, header: the variable-block-size bit; a sample-rate code other than 0.
//   5. CRC16 over all bytes in front of the last two.  It comes before any subframe is parsed, so a frame damaged in storage is CRC8 or
//      CRC16 and rules 6 to 8 are met only by frames whose CRCs are right.  (A caller that does not know the frame's size -- rule 10 --
//      cannot check it here.)
//   6. The subframes: parsing ends at the first of these two, in the order of the bitstream:
//        SYNTAX       the subframe's first bit is 1; a reserved subframe type (00001x, 0001xx, 001ooo with o > 4, 01xxxx); an order
//                     above n; LPC precision code 1111; a negative LPC shift (16 .. 31 of the 5-bit field); Rice method 1x; a partition
//                     order p with n % 2^p != 0 or (n >> p) below the predictor order; the bits run out
//        UNSUPPORTED  a constant subframe; wasted bits; Rice method 00; an escape partition (parameter 31)
//      A subframe is: 0, tttttt, w; verbatim (000001): n samples; fixed (001ooo): o warm-up samples; LPC (1ppppp, order p + 1): the
//      warm-up samples, precision - 1 in 4 bits, shift in 5, the coefficients; then for fixed and LPC the method `01`, pppp, and per
//      partition kkkkk and its Rice codes.  Sample sizes: the depth, one bit more for a side channel.
//      x(i) = prediction + r(i): 0, x1, 2 x1 - x2, 3 x1 - 3 x2 + x3, 4 x1 - 6 x2 + 4 x3 - x4 for the fixed orders,
//      (sum of q[j] x(i - j)) >> shift for LPC, all in 64 bits (|q| < 2^14, |x| <= 2^24, 32 terms; a Rice code holds at most
//      2^20 zeros and 30 low bits).
//   7. LENGTH: the bits up to the next byte boundary are not zero; the subframes do not end two bytes in front of the frame's end.
//   8. SAMPLES, the last reason: the frame parses from its first bit to its last, and a decoded sample does not fit the subframe's
//      sample size (it is then wrapped to that size, so that the arithmetic stays bounded), is not the PCM's (the verifier), or gives
//      a left or right sample that does not fit the depth (the decoder's stereo reconstruction).  A wrong sample does not end the
//      parse: a frame whose codes also overrun or underrun it is SYNTAX or LENGTH.
//   9. The verifier compares in the domain of the coded signals: mid = (L + R) >> 1 and side = L - R formed from the PCM as rule 2 of
//      flac_frame_enc.h forms them ((L, R) -> (M, S) is injective).  The prediction runs on what was decoded; up to the first mismatch
//      that IS the original.
//  10. A caller without a size table (d2d_flac_decode_host; d2d_flac_verify_host with sizes = NULL) finds the frame's end by parsing:
//      rules 2 to 4, 6, the padding of rule 7, then two more bytes must exist (else SYNTAX) and be the CRC-16 (rule 5).  At most
//      D2D_FLAC_FRAME_BOUND(4096) bytes are looked at for one frame.
// Every loop is bounded by n, by the order, by 2^p <= n or by the bits that are left: the parser ends on any bytes, and the bit reader
// never reads outside [p, p + size).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/dsd2dxd_amd.h"

#if defined(__HIPCC__)
#define D2D_PARSE_HD __host__ __device__ __forceinline__
#else
#define D2D_PARSE_HD inline
#endif

namespace d2dparse {

constexpr uint32_t MAX_LPC_ORDER = 32;         // the ring and the coefficient storage a caller hands in hold this many words each
constexpr uint32_t MAX_HEADER = 17;            // 4 + 7 (a 36-bit sample number) + 2 (block size) + 2 (sample rate) + 1 (CRC-8), and one to spare

// `nb` (1 .. 4) bytes at p, big-endian, in the low bits; an aligned group of four is one load
D2D_PARSE_HD uint32_t load_be(const uint8_t* p, uint32_t nb) {
    if (nb == 4 && ((uintptr_t)p & 3) == 0) { uint32_t w; __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4); return __builtin_bswap32(w); }
    uint32_t v = 0;
    for (uint32_t i = 0; i < nb; ++i) v = (v << 8) | p[i];
    return v;
}

// MSB-first reader over [p + begin, p + end): it never touches a byte outside, whatever the bits say.  Running out of bits raises
// `bad` (and yields zeros): a syntax error, not a read.  It reads single bytes up to the first 4-byte boundary of the address, then
// aligned words, then the last bytes: frames start anywhere in `out`.
struct BitReader {
    const uint8_t* p;
    uint32_t pos, end;                         // the next byte to load; one past the last
    uint64_t window = 0;                       // the next bits at the top; zeros below the `nbits` valid ones
    uint32_t nbits = 0;
    bool bad = false;
    D2D_PARSE_HD BitReader(const uint8_t* p_, uint32_t begin, uint32_t end_) : p(p_), pos(begin), end(end_ > begin ? end_ : begin) {}
    D2D_PARSE_HD void refill() {
        while (nbits <= 32 && pos < end) {
            const uint32_t to_boundary = 4u - (uint32_t)((uintptr_t)(p + pos) & 3u), left = end - pos;
            const uint32_t nb = to_boundary < left ? to_boundary : left;
            window |= (uint64_t)load_be(p + pos, nb) << (64 - nbits - 8 * nb);
            nbits += 8 * nb; pos += nb;
        }
    }
    D2D_PARSE_HD void consume(uint32_t n) { window = n >= 64 ? 0 : window << n; nbits -= n; }
    // n = 0 .. 32 bits
    D2D_PARSE_HD uint32_t read(uint32_t n) {
        if (n == 0) return 0;
        if (nbits < n) refill();
        if (nbits < n) { bad = true; nbits = 0; window = 0; return 0; }
        const uint32_t v = (uint32_t)(window >> (64 - n));
        consume(n);
        return v;
    }
    // n = 1 .. 32 bits, two's complement
    D2D_PARSE_HD int32_t sread(uint32_t n) {
        const uint32_t v = read(n);
        return n >= 32 ? (int32_t)v : (int32_t)(v ^ (1u << (n - 1))) - (int32_t)(1u << (n - 1));
    }
    // the zeros in front of the next 1, which is consumed too: a leading-zero count on the window, continued over refills; the run is
    // bounded by the bits that remain
    D2D_PARSE_HD uint32_t unary() {
        uint32_t zeros = 0;
        for (;;) {
            if (nbits == 0 || window == 0) {
                zeros += nbits; nbits = 0; window = 0;
                if (pos >= end) { bad = true; return 0; }
                refill();
                continue;
            }
            const uint32_t lz = (uint32_t)__builtin_clzll(window);      // below nbits: the bits under the valid ones are zero
            zeros += lz;
            consume(lz + 1);
            return zeros;
        }
    }
    D2D_PARSE_HD uint32_t bits_used(uint32_t begin) const { return 8 * (pos - begin) - nbits; }
    D2D_PARSE_HD uint32_t byte_pos() const { return pos - nbits / 8; }  // after align(): the next unread byte
};

// the tables' entries (the encoders' polynomials: x^8 + x^2 + x + 1, x^16 + x^15 + x^2 + 1)
D2D_PARSE_HD uint32_t crc8_step(uint32_t c, uint32_t byte) {
    c ^= byte;
    for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}
D2D_PARSE_HD uint32_t crc16_entry(uint32_t i) {
    uint32_t c = i << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    return c;
}
// CRC-16 of [p, p + len) with a 256-entry table (the host's static one, the kernel's copy in LDS); bytes, aligned words, bytes
D2D_PARSE_HD uint32_t crc16(const uint8_t* p, uint32_t len, const uint16_t* tab) {
    uint32_t c = 0, i = 0;
    for (; i < len && ((uintptr_t)(p + i) & 3u); ++i) c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ p[i]];
    for (; i + 4 <= len; i += 4) {
        const uint32_t w = load_be(p + i, 4);
        c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ (w >> 24)];
        c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ ((w >> 16) & 0xFFu)];
        c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ ((w >> 8) & 0xFFu)];
        c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ (w & 0xFFu)];
    }
    for (; i < len; ++i) c = ((c << 8) & 0xFFFFu) ^ tab[(c >> 8) ^ p[i]];
    return c;
}

struct Expect { uint32_t channels, depth, n, frame_no; };           // n = 0: any block size up to 4096
struct Header { uint32_t n, assignment, bytes; };                   // what the header says; its length with the CRC-8

// rules 2 to 4 on the frame at p, of which `avail` bytes may be read
D2D_PARSE_HD uint32_t parse_header(const uint8_t* p, uint32_t avail, const Expect& ex, Header& h) {
    BitReader br(p, 0, avail < MAX_HEADER ? avail : MAX_HEADER);
    const uint32_t sync = br.read(16), bs_code = br.read(4), rate_code = br.read(4), assignment = br.read(4), size_code = br.read(3), reserved = br.read(1);
    if (br.bad || (sync & 0xFFFEu) != 0xFFF8u || bs_code == 0 || rate_code == 15 || assignment > 10 || size_code == 3 || reserved) return D2D_FLAC_BAD_HEADER;
    const bool variable = sync & 1u;
    // the frame number: 0xxxxxxx, or 110xxxxx .. 1111110x (11111110 with a sample number) and that many 10xxxxxx
    const uint32_t lead = br.read(8);
    uint32_t extra = 0;
    while (extra < 8 && (lead & (0x80u >> extra))) ++extra;          // the ones in front
    if (extra == 1 || extra > (variable ? 6u : 5u) + 1u) return D2D_FLAC_BAD_HEADER;
    if (extra) --extra;                                              // the bytes that follow
    uint64_t number = extra ? lead & (0x3Fu >> extra) : lead;
    for (uint32_t i = 0; i < extra; ++i) {
        const uint32_t b = br.read(8);
        if ((b & 0xC0u) != 0x80u) return D2D_FLAC_BAD_HEADER;
        number = (number << 6) | (b & 0x3Fu);
    }
    uint32_t n = bs_code == 1 ? 192 : bs_code <= 5 ? 576u << (bs_code - 2) : bs_code == 6 ? br.read(8) + 1 : bs_code == 7 ? br.read(16) + 1 : 256u << (bs_code - 8);
    if (rate_code == 12) (void)br.read(8);
    if (rate_code == 13 || rate_code == 14) (void)br.read(16);
    const uint32_t crc = br.read(8);
    if (br.bad) return D2D_FLAC_BAD_HEADER;
    h.n = n; h.assignment = assignment; h.bytes = br.byte_pos();
    const uint32_t channels = assignment < 8 ? assignment + 1 : 2, depth = size_code == 4 ? 16 : size_code == 5 ? 20 : size_code == 6 ? 24 : 0;
    if ((ex.n ? n != ex.n : n > D2D_FLAC_BLOCK) || channels != ex.channels || depth != ex.depth || (!variable && number != ex.frame_no)) return D2D_FLAC_BAD_HEADER;
    uint32_t c = 0;
    for (uint32_t i = 0; i + 1 < h.bytes; ++i) c = crc8_step(c, p[i]);
    if (c != crc) return D2D_FLAC_BAD_CRC8;
    if (variable || rate_code != 0) return D2D_FLAC_BAD_UNSUPPORTED;
    return D2D_FLAC_BAD_NONE;
}

// One subframe of n samples of `bps` bits (rule 6).  Sig takes the samples: bool put(i, v) -- false: not the expected sample, which
// raises `wrong` (rule 8) -- and lends the storage of an LPC subframe: int32_t& hist(k), int32_t& coef(k), k < MAX_LPC_ORDER.
template <class Sig>
D2D_PARSE_HD uint32_t parse_subframe(BitReader& br, uint32_t n, uint32_t bps, Sig& sig, bool& wrong) {
    const uint32_t head = br.read(8);
    if (br.bad || (head & 0x80u)) return D2D_FLAC_BAD_SYNTAX;
    const uint32_t type = (head >> 1) & 0x3Fu;
    uint32_t order = 0;
    bool lpc = false;
    if (type == 0) return D2D_FLAC_BAD_UNSUPPORTED;                  // constant
    if (type >= 32) { lpc = true; order = type - 31; }
    else if (type >= 16) return D2D_FLAC_BAD_SYNTAX;
    else if (type >= 8) { order = type - 8; if (order > 4) return D2D_FLAC_BAD_SYNTAX; }
    else if (type != 1) return D2D_FLAC_BAD_SYNTAX;
    if (head & 1u) return D2D_FLAC_BAD_UNSUPPORTED;                  // wasted bits
    if (type == 1) {                                                 // verbatim
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t v = br.sread(bps);
            if (br.bad) return D2D_FLAC_BAD_SYNTAX;
            if (!sig.put(i, v)) wrong = true;
        }
        return D2D_FLAC_BAD_NONE;
    }
    if (order > n) return D2D_FLAC_BAD_SYNTAX;
    int64_t x1 = 0, x2 = 0, x3 = 0, x4 = 0;                          // x(i - 1) .. x(i - 4): all a fixed predictor needs
    for (uint32_t i = 0; i < order; ++i) {
        const int32_t v = br.sread(bps);
        if (br.bad) return D2D_FLAC_BAD_SYNTAX;
        if (!sig.put(i, v)) wrong = true;
        x4 = x3; x3 = x2; x2 = x1; x1 = v;
        if (lpc) sig.hist(i & (MAX_LPC_ORDER - 1)) = v;
    }
    uint32_t shift = 0;
    if (lpc) {
        const uint32_t precision = br.read(4) + 1;
        shift = br.read(5);
        if (br.bad || precision == 16 || shift >= 16) return D2D_FLAC_BAD_SYNTAX;
        for (uint32_t j = 0; j < order; ++j) sig.coef(j) = br.sread(precision);
        if (br.bad) return D2D_FLAC_BAD_SYNTAX;
    }
    const uint32_t method = br.read(2), porder = br.read(4);
    if (br.bad || method >= 2) return D2D_FLAC_BAD_SYNTAX;
    if (method == 0) return D2D_FLAC_BAD_UNSUPPORTED;
    const uint32_t psz = n >> porder;
    if ((n & ((1u << porder) - 1)) || psz < order) return D2D_FLAC_BAD_SYNTAX;
    const int64_t lo = -((int64_t)1 << (bps - 1)), hi = ((int64_t)1 << (bps - 1)) - 1;
    uint32_t i = order;
    for (uint32_t j = 0; j < (1u << porder); ++j) {
        const uint32_t k = br.read(5);
        if (br.bad) return D2D_FLAC_BAD_SYNTAX;
        if (k == 31) return D2D_FLAC_BAD_UNSUPPORTED;                // escape
        for (const uint32_t stop = (j + 1) * psz; i < stop; ++i) {
            const uint64_t q = br.unary();
            const uint64_t u = (q << k) | br.read(k);
            if (br.bad) return D2D_FLAC_BAD_SYNTAX;
            const int64_t r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
            int64_t pred;
            if (lpc) {
                int64_t sum = 0;
                for (uint32_t m = 0; m < order; ++m) sum += (int64_t)sig.coef(m) * sig.hist((i - 1 - m) & (MAX_LPC_ORDER - 1));
                pred = sum >> shift;
            } else pred = order == 0 ? 0 : order == 1 ? x1 : order == 2 ? 2 * x1 - x2 : order == 3 ? 3 * x1 - 3 * x2 + x3 : 4 * x1 - 6 * x2 + 4 * x3 - x4;
            int64_t v = pred + r;
            if (v < lo || v > hi) { wrong = true; v = (int64_t)((uint64_t)v << (64 - bps)) >> (64 - bps); }
            if (!sig.put(i, (int32_t)v)) wrong = true;
            if (lpc) sig.hist(i & (MAX_LPC_ORDER - 1)) = (int32_t)v;
            else { x4 = x3; x3 = x2; x2 = x1; x1 = v; }
        }
    }
    return D2D_FLAC_BAD_NONE;
}

// Rules 2 to 8, or rule 10 where the size is not known: then `avail` is what may be read and *size_out the size found.  Sig also has
// void begin(s, assignment): subframe s of the frame starts.
template <class Sig>
D2D_PARSE_HD uint32_t parse_frame(const uint8_t* p, uint32_t avail, bool size_known, const Expect& ex, const uint16_t* crc_tab, Sig& sig,
                                  Header& h, uint32_t* size_out) {
    uint32_t reason = parse_header(p, avail, ex, h);
    if (reason) return reason;
    auto crc_ok = [&](uint32_t body_end) { return crc16(p, body_end, crc_tab) == (((uint32_t)p[body_end] << 8) | p[body_end + 1]); };
    const uint32_t body_end = !size_known ? avail : avail - 2 > h.bytes ? avail - 2 : h.bytes;       // (a header has 6 bytes at least)
    if (size_known && !crc_ok(avail - 2)) return D2D_FLAC_BAD_CRC16;
    BitReader br(p, h.bytes, body_end);
    const uint32_t channels = h.assignment < 8 ? h.assignment + 1 : 2;
    bool wrong = false;
    for (uint32_t s = 0; s < channels; ++s) {
        const bool side = (h.assignment == 8 && s == 1) || (h.assignment == 9 && s == 0) || (h.assignment == 10 && s == 1);
        sig.begin(s, h.assignment);
        reason = parse_subframe(br, h.n, ex.depth + (side ? 1 : 0), sig, wrong);
        if (reason) return reason;
    }
    if (br.read((8 - br.bits_used(h.bytes) % 8) % 8) != 0) return D2D_FLAC_BAD_LENGTH;
    const uint32_t at = br.byte_pos();
    if (size_known) { if (at != avail - 2 || at < h.bytes) return D2D_FLAC_BAD_LENGTH; }
    else {
        if (at + 2 > avail) return D2D_FLAC_BAD_SYNTAX;
        if (!crc_ok(at)) return D2D_FLAC_BAD_CRC16;
        *size_out = at + 2;
    }
    return wrong ? D2D_FLAC_BAD_SAMPLES : D2D_FLAC_BAD_NONE;
}

// sample `idx` of packed little-endian PCM as the encoders read it: 16 bits in 2 bytes, 24 in 3, 20 as the 3-byte container >> 4
D2D_PARSE_HD int32_t pcm_sample(const uint8_t* pcm, size_t idx, uint32_t depth) {
    if (depth == 16) { const uint8_t* q = pcm + idx * 2; return (int16_t)(q[0] | (q[1] << 8)); }
    const uint8_t* q = pcm + idx * 3;
    const int32_t v = (int32_t)((uint32_t)(q[0] | (q[1] << 8) | (q[2] << 16)) << 8) >> 8;
    return depth == 20 ? v >> 4 : v;
}

// The verifier's Sig (rule 9): compares each decoded sample with the coded signal formed from the block's PCM.  `store` holds
// 2 * MAX_LPC_ORDER words, word k at store[k * stride]: the history ring, then the coefficients.
struct VerifySig {
    const uint8_t* pcm;                        // the block's first frame
    uint32_t channels, depth, stride;
    int32_t* store;
    uint32_t kind = 0, c = 0;                  // 0: channel c; 1: mid; 2: side
    D2D_PARSE_HD void begin(uint32_t s, uint32_t assignment) {
        kind = 0; c = s;
        if (assignment >= 8) { const bool side = assignment == 9 ? s == 0 : s == 1; kind = side ? 2 : assignment == 10 ? 1 : 0; }
    }
    D2D_PARSE_HD bool put(uint32_t i, int32_t v) const {
        if (kind == 0) return v == pcm_sample(pcm, (size_t)i * channels + c, depth);
        const int32_t l = pcm_sample(pcm, (size_t)i * 2, depth), r = pcm_sample(pcm, (size_t)i * 2 + 1, depth);
        return v == (kind == 1 ? (l + r) >> 1 : l - r);
    }
    D2D_PARSE_HD int32_t& hist(uint32_t k) const { return store[k * stride]; }
    D2D_PARSE_HD int32_t& coef(uint32_t k) const { return store[(MAX_LPC_ORDER + k) * stride]; }
};

// One block of a verify call behind rule 1: the frame at `frame`, `size` bytes (or, with size_known false, at most that many), against
// the n frames of PCM at `pcm`.  Returns the reason; *size_out as parse_frame.
D2D_PARSE_HD uint32_t verify_frame(const uint8_t* frame, uint32_t size, bool size_known, const Expect& ex, const uint8_t* pcm,
                                   const uint16_t* crc_tab, int32_t* store, uint32_t stride, uint32_t* size_out) {
    VerifySig sig{pcm, ex.channels, ex.depth, stride, store};
    Header h;
    return parse_frame(frame, size, size_known, ex, crc_tab, sig, h, size_out);
}

// rule 1 for block b of `blocks` at offset `off` of a file of bytes_out bytes
D2D_PARSE_HD bool size_ok(uint64_t off, uint32_t size, uint64_t bytes_out, uint32_t bound, bool last) {
    return size != 0 && size <= bound && off + size <= bytes_out && (!last || off + size == bytes_out);
}

// the status word of a block: the reason, and above it n where the block is good
D2D_PARSE_HD uint32_t status_word(uint32_t reason, uint32_t n) { return reason ? reason : n << 8; }

}  // namespace d2dparse
