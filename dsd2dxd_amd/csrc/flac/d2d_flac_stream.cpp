// d2d_flac_stream.cpp -- d2d_convert_stream_flac: a whole DSD stream to FLAC frames through the public calls (d2d_translate_batch_device,
// d2d_flac_encode_device_effort, for the verified twin d2d_flac_verify_device, for the hashing one d2d_flac_md5_*_device, for the measuring one d2d_loud_measure_device and d2d_true_peak_measure_device) and HIP's host API.  Host code: it launches no kernel.
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <algorithm>
#include "d2d_flac_internal.h"
#include "../loud/d2d_loud_internal.h"

using namespace d2dflac;

namespace {

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { bytes = n; return hipMalloc(&p, std::max<size_t>(n, 16)); }
};
struct PinBuf {
    void* p = nullptr;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc(&p, std::max<size_t>(n, 16), hipHostMallocDefault); }
};
// All device work of the stream driver goes to the null stream: the engine remembers the stream of its last call (d2d_peak waits on
// it), so it must not be one that ends with this function.  (The buffers' release waits for the device.)
struct Stream { hipStream_t s = nullptr; };

}  // namespace

#define FLAC_HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, what); } while (0)

extern "C" int d2d_convert_stream_flac(d2d_engine* e, uint32_t bit_depth, d2d_read_fn read, void* ru, d2d_write_fn write, void* wu,
                                       const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                       uint64_t total, size_t chunk, d2d_flac_stream_stats* stats) {
    return d2d_convert_stream_flac_effort(e, bit_depth, D2D_FLAC_EFFORT_FIXED2, read, ru, write, wu, cancel, progress, pu, total, chunk, stats);
}

// the driver behind the twins; `check` non-null: every chunk's frames are verified on the device before `write` sees them; `md5` non-null:
// every chunk's new frames are hashed on the device and the digest is written there after the last; `loud` non-null: every chunk's new
// sub-blocks are measured on the device and their cells go into the meter
static int convert_stream_flac(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                               d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                               uint64_t total, size_t chunk, d2d_flac_stream_stats* stats, d2d_flac_check* check, uint8_t* md5, d2d_loud* loud);

extern "C" int d2d_convert_stream_flac_effort(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                                              d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                              uint64_t total, size_t chunk, d2d_flac_stream_stats* stats) {
    return convert_stream_flac(e, bit_depth, effort, read, ru, write, wu, cancel, progress, pu, total, chunk, stats, nullptr, nullptr, nullptr);
}

extern "C" int d2d_convert_stream_flac_verified(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                                                d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                                uint64_t total, size_t chunk, d2d_flac_stream_stats* stats, d2d_flac_check* check) {
    if (!check) return fail(D2D_ERR_PARAM, "null check record");
    return convert_stream_flac(e, bit_depth, effort, read, ru, write, wu, cancel, progress, pu, total, chunk, stats, check, nullptr, nullptr);
}

extern "C" int d2d_convert_stream_flac_md5(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                                           d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                           uint64_t total, size_t chunk, d2d_flac_stream_stats* stats, d2d_flac_check* check, uint8_t md5[16]) {
    if (!md5) return fail(D2D_ERR_PARAM, "null md5");
    return convert_stream_flac(e, bit_depth, effort, read, ru, write, wu, cancel, progress, pu, total, chunk, stats, check, md5, nullptr);
}

extern "C" int d2d_convert_stream_flac_loud(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                                            d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                                            uint64_t total, size_t chunk, d2d_flac_stream_stats* stats, d2d_flac_check* check, uint8_t md5[16],
                                            d2d_loud* loud) {
    if (!loud) return fail(D2D_ERR_PARAM, "null meter");
    return convert_stream_flac(e, bit_depth, effort, read, ru, write, wu, cancel, progress, pu, total, chunk, stats, check, md5, loud);
}

static int convert_stream_flac(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* ru,
                               d2d_write_fn write, void* wu, const volatile int* cancel, d2d_progress_fn progress, void* pu,
                               uint64_t total, size_t chunk, d2d_flac_stream_stats* stats, d2d_flac_check* check, uint8_t* md5, d2d_loud* loud) {
    if (!effort_ok(effort)) return fail(D2D_ERR_PARAM, EFFORT_MESSAGE);
    if (!e) return fail(D2D_ERR_PARAM, "null engine");
    if (!read) return fail(D2D_ERR_PARAM, "null read callback");
    if (!stats) return fail(D2D_ERR_PARAM, "null stats");
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    const size_t fb = d2d_frame_bytes(e), sb = sample_bytes(bit_depth);
    if (fb == 0 || fb % sb || fb / sb > 8) return fail(D2D_ERR_PARAM, "the engine's frames do not hold 1 to 8 channels of this bit depth");
    const uint32_t ch = (uint32_t)(fb / sb);
    const uint32_t in_ch = d2d_input_channels(e);      // the reads and uploads move whole INPUT frames: wider than the PCM's on a mixed or channel-subset engine
    if (chunk == 0) chunk = 1u << 22;
    // the engine's device becomes this thread's current device (d2d_peak selects it and waits for the engine's pending work)
    double peak0 = 0.0;
    if (d2d_peak(e, 0, 0, &peak0) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
    *stats = d2d_flac_stream_stats{0, 0, 0, 0};
    if (check) *check = d2d_flac_check{0, 0, 0, 0xFFFFFFFFu, D2D_FLAC_BAD_NONE};

    // frames one chunk can add: the engine's own count for a chunk from where it stands, and a margin for the rounding of later ones
    const size_t chunk_frames = d2d_next_frames(e, 0, chunk) + 64, cap_frames = chunk_frames + BS;
    const size_t out_cap = d2d_flac_bound_bytes(ch, bit_depth, cap_frames, 1), ws_cap = d2d_flac_workspace_bytes(ch, bit_depth, cap_frames, 1);
    Stream st;
    PinBuf h_in[2], h_out, h_res, h_chk;
    DevBuf d_in, d_new, d_pcm, d_out, d_ws;
    FLAC_HIP(h_in[0].alloc(chunk * in_ch), "hipHostMalloc"); FLAC_HIP(h_in[1].alloc(chunk * in_ch), "hipHostMalloc");
    FLAC_HIP(h_out.alloc(out_cap), "hipHostMalloc"); FLAC_HIP(h_res.alloc(sizeof(d2d_flac_result)), "hipHostMalloc");
    FLAC_HIP(d_in.alloc(chunk * in_ch), "hipMalloc"); FLAC_HIP(d_new.alloc(chunk_frames * fb), "hipMalloc");
    FLAC_HIP(d_pcm.alloc(cap_frames * fb), "hipMalloc"); FLAC_HIP(d_out.alloc(out_cap), "hipMalloc"); FLAC_HIP(d_ws.alloc(ws_cap), "hipMalloc");
    d2d_flac_result* res = (d2d_flac_result*)h_res.p;
    if (check) FLAC_HIP(h_chk.alloc(sizeof(d2d_flac_check)), "hipHostMalloc");
    d2d_flac_check* chk = (d2d_flac_check*)h_chk.p;
    // the hash: one state record on the device, the digest in pinned memory
    DevBuf d_md5; PinBuf h_dig;
    if (md5) {
        FLAC_HIP(d_md5.alloc(sizeof(d2d_flac_md5_state)), "hipMalloc"); FLAC_HIP(h_dig.alloc(16), "hipHostMalloc");
        const int mrc = d2d_flac_md5_init_device(d_md5.p, 1, st.s);
        if (mrc != D2D_OK) return mrc;
    }
    // the meter: a PCM buffer of its own that keeps the pre-roll of the next sub-block (two sub-blocks, and what has come of the third) in
    // front of each chunk's frames -- the encoder's carry stays what it was -- and the cells in pinned memory the kernel writes directly.
    // What is kept moves to the front through the second buffer (the ranges may overlap).
    if (loud && d2dloud::meter_channels(loud) != ch) return fail(D2D_ERR_PARAM, "the meter was created for another channel count than the engine's");
    const uint32_t rate = loud ? d2dloud::meter_rate(loud) : 0;
    const size_t S = rate / 10, l_cap = 3 * S + chunk_frames, l_rows = S ? l_cap / S + 2 : 0;
    DevBuf d_loud[2]; PinBuf h_cells, h_peaks;
    if (loud) {
        FLAC_HIP(d_loud[0].alloc(l_cap * fb), "hipMalloc"); FLAC_HIP(d_loud[1].alloc(l_cap * fb), "hipMalloc");
        FLAC_HIP(h_cells.alloc(l_rows * ch * sizeof(d2d_loud_cell)), "hipHostMalloc");
    }
    // a meter whose true peak was switched on (d2d_loud_set_true_peak): the same rows once more, as doubles, over the same buffer --
    // what holds the pre-roll holds the eleven frames of history
    const bool tpeak = loud && d2dloud::meter_true_peak(loud);
    if (tpeak) FLAC_HIP(h_peaks.alloc(l_rows * ch * sizeof(double)), "hipHostMalloc");
    uint64_t l_first = 0, l_next = 0;  // the stream position of d_loud[l_cur]'s first frame; the next sub-block to measure
    size_t l_have = 0;                 // frames in d_loud[l_cur]
    int l_cur = 0;

    size_t carry = 0;                 // frames in front of d_pcm that no block has taken yet
    uint64_t done = 0;
    int cur = 0;
    long got = read(ru, (uint8_t*)h_in[cur].p, chunk);
    if (got < 0) return fail(D2D_ERR_IO, "read callback failed");
    while (got > 0) {
        if (cancel && *cancel) return fail(D2D_ERR_CANCELLED, "Conversion cancelled");
        const size_t L = (size_t)got;
        if (L > chunk) return fail(D2D_ERR_IO, "read callback returned more than it was asked for");
        // upload and convert; the PCM lands in a buffer of its own (the translate call wants 16-byte alignment, the end of the carry
        // has none) and is copied behind the carry on the same stream
        d2d_file_io tio{};
        tio.dsd = d_in.p; tio.bytes_per_channel = L; tio.pcm = d_new.p; tio.pcm_capacity_bytes = d_new.bytes;
        FLAC_HIP(hipMemcpyAsync(d_in.p, h_in[cur].p, L * in_ch, hipMemcpyHostToDevice, st.s), "hipMemcpyAsync");
        if (d2d_translate_batch_device(e, &tio, 1, st.s) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
        const size_t nf = tio.frames_out;
        if (md5) {                                                    // the chunk's new frames, where the translate call left them
            const d2d_flac_md5_io mio{d_new.p, nf};
            const int mrc = d2d_flac_md5_update_device(ch, bit_depth, &mio, 1, d_md5.p, st.s);
            if (mrc != D2D_OK) return mrc;
        }
        if (carry + nf > cap_frames) return fail(D2D_ERR_STATE, "a chunk produced more frames than planned");
        if (nf) FLAC_HIP(hipMemcpyAsync((uint8_t*)d_pcm.p + carry * fb, d_new.p, nf * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
        // the next chunk is read while the GPU works: the stream ends with this chunk if there is none
        const long next = read(ru, (uint8_t*)h_in[cur ^ 1].p, chunk);
        if (next < 0) return fail(D2D_ERR_IO, "read callback failed");
        d2d_loud_io lio{};
        if (loud) {                                                   // the chunk's frames behind the kept ones; every sub-block they complete
            if (l_have + nf > l_cap) return fail(D2D_ERR_STATE, "a chunk produced more frames than planned");
            if (nf) FLAC_HIP(hipMemcpyAsync((uint8_t*)d_loud[l_cur].p + l_have * fb, d_new.p, nf * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
            l_have += nf;
            lio.pcm = d_loud[l_cur].p; lio.frames = l_have; lio.first_frame = l_first; lio.first_subblock = l_next; lio.final = next == 0;
            lio.cells = (d2d_loud_cell*)h_cells.p; lio.cells_capacity = l_rows * ch; lio.next_subblock = l_next;
            const int lrc = d2d_loud_measure_device(ch, bit_depth, rate, &lio, 1, st.s);
            if (lrc != D2D_OK) return lrc;
        }
        d2d_tpeak_io pio{};
        if (tpeak) {
            pio.pcm = lio.pcm; pio.frames = lio.frames; pio.first_frame = lio.first_frame; pio.first_subblock = lio.first_subblock; pio.final = lio.final;
            pio.peaks = (double*)h_peaks.p; pio.peaks_capacity = l_rows * ch; pio.next_subblock = l_next;
            const int prc = d2d_true_peak_measure_device(ch, bit_depth, rate, &pio, 1, st.s);
            if (prc != D2D_OK) return prc;
        }
        d2d_flac_io fio{};
        fio.pcm = d_pcm.p; fio.frames = carry + nf; fio.first_block = (uint32_t)stats->blocks; fio.final = next == 0;
        fio.out = d_out.p; fio.out_capacity_bytes = d_out.bytes; fio.result = res;
        if (stats->blocks > 0xFFFFFFFFull) return fail(D2D_ERR_PARAM, "frame numbers are 31 bits");
        const int rc = d2d_flac_encode_device_effort(ch, bit_depth, effort, &fio, 1, d_ws.p, d_ws.bytes, st.s);
        if (rc != D2D_OK) return rc;
        if (check) {
            const int vrc = d2d_flac_verify_device(ch, bit_depth, &fio, 1, d_ws.p, d_ws.bytes, chk, st.s);
            if (vrc != D2D_OK) return vrc;
        }
        FLAC_HIP(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        const d2d_flac_result r = *res;
        if (check) {                                                  // the record comes with the result; a bad block keeps its chunk from `write`
            check->samples_checked += chk->samples_checked; check->blocks_checked += chk->blocks_checked;
            if (chk->bad_blocks) {
                if (!check->bad_blocks) { check->first_bad_block = (uint32_t)stats->blocks + chk->first_bad_block; check->first_bad_reason = chk->first_bad_reason; }
                check->bad_blocks += chk->bad_blocks;
                return fail(D2D_ERR_VERIFY, "FLAC verify failed: block " + std::to_string(check->first_bad_block) + " (" + reason_name(check->first_bad_reason) + ")");
            }
        }
        if (loud) {                                                   // the cells came with the result
            const int lrc = d2d_loud_add(loud, lio.cells, lio.subblocks, lio.cells_out > lio.subblocks * ch);
            if (lrc != D2D_OK) return lrc;
            if (tpeak) {
                const int prc = d2d_loud_add_true_peaks(loud, pio.peaks, pio.subblocks, pio.peaks_out > pio.subblocks * ch);
                if (prc != D2D_OK) return prc;
            }
            l_next = lio.next_subblock;
            const uint64_t keep_from = (l_next > 2 ? l_next - 2 : 0) * (uint64_t)S;     // the pre-roll of the next sub-block
            const size_t drop = (size_t)(keep_from - l_first);
            if (drop) {
                l_have -= drop;
                if (l_have) FLAC_HIP(hipMemcpyAsync(d_loud[l_cur ^ 1].p, (uint8_t*)d_loud[l_cur].p + drop * fb, l_have * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
                l_cur ^= 1; l_first = keep_from;
            }
        }
        if (r.bytes_out) {
            FLAC_HIP(hipMemcpy(h_out.p, d_out.p, r.bytes_out, hipMemcpyDeviceToHost), "hipMemcpy");
            if (write && write(wu, h_out.p, r.bytes_out) != 0) return fail(D2D_ERR_IO, "write callback failed");
        }
        if (fio.blocks) {
            stats->min_frame_bytes = stats->blocks ? std::min(stats->min_frame_bytes, r.min_frame_bytes) : r.min_frame_bytes;
            stats->max_frame_bytes = std::max(stats->max_frame_bytes, r.max_frame_bytes);
            stats->blocks += fio.blocks;
            stats->samples_per_channel += fio.frames_consumed;
        }
        // the remainder moves to the front (it lies wholly behind its destination: a block was taken, or nothing moves)
        carry = fio.frames - fio.frames_consumed;
        if (carry && fio.frames_consumed)
            FLAC_HIP(hipMemcpyAsync(d_pcm.p, (uint8_t*)d_pcm.p + fio.frames_consumed * fb, carry * fb, hipMemcpyDeviceToDevice, st.s), "hipMemcpyAsync");
        done += (uint64_t)L;
        if (progress && total) {
            float pct = (float)(100.0 * (double)done / (double)total);
            if (pct >= 100.0f) pct = 99.99f;       // exactly 100 is reserved for the end
            progress(pu, pct);
        }
        got = next; cur ^= 1;
    }
    if (md5) {
        const int mrc = d2d_flac_md5_final_device(d_md5.p, 1, h_dig.p, st.s);
        if (mrc != D2D_OK) return mrc;
        FLAC_HIP(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        memcpy(md5, h_dig.p, 16);
    }
    if (progress) progress(pu, 100.0f);
    return D2D_OK;
}
