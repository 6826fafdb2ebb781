// d2d_loud_internal.h -- what the host and the device side of the loudness calls (include/dsd2dxd_amd.h, "Loudness where the PCM is")
// share besides the arithmetic of loud_meter.h: the checks and the counts of one file of a call.  Host code only.
#pragma once
#include "../flac/d2d_flac_internal.h"
#include "loud_meter.h"
#include "true_peak.h"

namespace d2dloud {

using d2dflac::fail;

constexpr uint64_t MAX_SUBBLOCK = (uint64_t)1 << 40;               // sub-block numbers, so that frame numbers stay far inside 64 bits
constexpr uint64_t MAX_FRAMES = (uint64_t)1 << 56;                 // frames of one call
constexpr uint64_t MAX_CELLS = (uint64_t)1 << 31;                  // cells of one file of one call

// the ten doubles of a rate, computed on the host (d2d_loud_host.cpp): the device receives them in its kernel arguments
Coef host_coefficients(uint32_t rate);

// what a meter was created for (the stream driver measures at the meter's rate)
uint32_t meter_rate(const d2d_loud* h);
uint32_t meter_channels(const d2d_loud* h);
bool meter_true_peak(const d2d_loud* h);                           // d2d_loud_set_true_peak(h, 1) was called

// what one file of a call measures
struct Plan {
    uint64_t S = 0;                                                // frames of a sub-block
    uint64_t whole = 0;                                            // whole sub-blocks from first_subblock on
    uint64_t partial_frames = 0;                                   // frames of the partial row of a final call, 0: none
    uint64_t rows() const { return whole + (partial_frames ? 1 : 0); }
};

// the checks of a call that do not look at a file
inline int check_call(uint32_t channels, uint32_t bit_depth, uint32_t rate) {
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "loudness is measured on 16, 20 or 24-bit integers or 32-bit floats (Invalid bit depth)");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "loudness is measured on 1 to 8 channels (Invalid channel count)");
    if (!rate_ok(rate)) return fail(D2D_ERR_PARAM, "loudness is measured at rates that are a multiple of 10 in 8000 .. 1411200");
    return D2D_OK;
}

// the rows of one file: p.S is set; every whole sub-block from first_subblock on that the buffer holds, and a final call's partial one
inline void count_rows(uint64_t first_frame, uint64_t frames, uint64_t first_subblock, int32_t final, Plan& p) {
    const uint64_t end = first_frame + frames, have = end / p.S;
    p.whole = have > first_subblock ? have - first_subblock : 0;
    const uint64_t measured_to = (first_subblock + p.whole) * p.S;
    p.partial_frames = (final && end > measured_to) ? end - measured_to : 0;
}

// the checks and the counts of one file with frames > 0; align: the alignment pcm and cells must have (the device call: 16, the host twin: 1)
inline int plan_file(const d2d_loud_io& io, uint32_t channels, uint32_t rate, uintptr_t align, Plan& p) {
    if (!io.pcm || !io.cells) return fail(D2D_ERR_PARAM, "pcm and cells must be non-null");
    if (((uintptr_t)io.pcm | (uintptr_t)io.cells) & (align - 1)) return fail(D2D_ERR_PARAM, "pcm and cells must be 16-byte aligned");
    if (io.frames > MAX_FRAMES || io.first_frame > MAX_FRAMES * 16 || io.first_subblock > MAX_SUBBLOCK)
        return fail(D2D_ERR_PARAM, "a stream position beyond what 64 bits of bytes hold");
    p.S = rate / 10;
    if (io.first_frame > start_subblock(io.first_subblock) * p.S)
        return fail(D2D_ERR_PARAM, "pcm does not hold the pre-roll: it must begin at or before frame max(0, first_subblock - 2) * rate / 10");
    count_rows(io.first_frame, io.frames, io.first_subblock, io.final, p);
    if (p.rows() * channels >= MAX_CELLS) return fail(D2D_ERR_PARAM, "more cells than one call writes; cut the call");
    if (p.rows() * channels > io.cells_capacity) return fail(D2D_ERR_CAPACITY, "cells_capacity is below the cells this call writes");
    return D2D_OK;
}

// the counts a successful call leaves in the record
inline void write_counts(d2d_loud_io& io, const Plan& p, uint32_t channels) {
    io.subblocks = (size_t)p.whole; io.cells_out = (size_t)(p.rows() * channels); io.next_subblock = io.first_subblock + p.whole;
}

// plan_file's sibling for the true-peak calls: the same rows and counts; the buffer must hold eleven frames of history instead of the
// pre-roll, and a cell is one double.  pcm_align, peaks_align: the device call 16 and 8, the host twin 1 and 1.
inline int plan_tpeak_file(const d2d_tpeak_io& io, uint32_t channels, uint32_t rate, uintptr_t pcm_align, uintptr_t peaks_align, Plan& p) {
    if (!io.pcm || !io.peaks) return fail(D2D_ERR_PARAM, "pcm and peaks must be non-null");
    if (((uintptr_t)io.pcm & (pcm_align - 1)) || ((uintptr_t)io.peaks & (peaks_align - 1)))
        return fail(D2D_ERR_PARAM, "pcm must be 16-byte aligned and peaks 8-byte aligned");
    if (io.frames > MAX_FRAMES || io.first_frame > MAX_FRAMES * 16 || io.first_subblock > MAX_SUBBLOCK)
        return fail(D2D_ERR_PARAM, "a stream position beyond what 64 bits of bytes hold");
    p.S = rate / 10;
    if (io.first_frame > d2dtp::history_start(io.first_subblock, p.S))
        return fail(D2D_ERR_PARAM, "pcm does not hold the history: it must begin at or before frame max(0, first_subblock * rate / 10 - 11)");
    count_rows(io.first_frame, io.frames, io.first_subblock, io.final, p);
    if (p.rows() * channels >= MAX_CELLS) return fail(D2D_ERR_PARAM, "more cells than one call writes; cut the call");
    if (p.rows() * channels > io.peaks_capacity) return fail(D2D_ERR_CAPACITY, "peaks_capacity is below the doubles this call writes");
    return D2D_OK;
}

inline void write_tpeak_counts(d2d_tpeak_io& io, const Plan& p, uint32_t channels) {
    io.subblocks = (size_t)p.whole; io.peaks_out = (size_t)(p.rows() * channels); io.next_subblock = io.first_subblock + p.whole;
}

}  // namespace d2dloud
