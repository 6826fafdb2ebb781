// d2d_flac_streams.cpp -- d2d_convert_streams_flac: the streams of an album in lockstep through one engine of n_files files
// (include/dsd2dxd_amd.h, "The batch driver").  d2d_flac_stream.cpp's driver for many files: the same public calls, each once per chunk
// for all files, the per-file copies of a chunk in one d2d_segments_move_device and the download of all files' frame bytes in one
// d2d_segments_pack_device.  Host code: it launches no kernel.
//
// WHAT DIFFERS FROM THE SINGLE DRIVER, and why the bytes do not.  Every length the moves need is host arithmetic known when the calls
// return (frames_out, frames_consumed, next_subblock); only bytes_out is the device's, and the pack reads it there.  So a chunk needs
// ONE synchronise.  The carried PCM of the encoder and of the meter each alternate between two buffers: what is kept goes to the
// front of the other buffer and the new frames behind it in the same move call, so no dst range overlaps a src range.  The calls
// see, per file, the frames the single driver shows them, cut at the same stream positions.
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "d2d_flac_internal.h"
#include "../loud/d2d_loud_internal.h"

using namespace d2dflac;

namespace {

struct DevBuf {
    uint8_t* p = nullptr; size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { bytes = n; return hipMalloc((void**)&p, std::max<size_t>(n, 16)); }
};
struct PinBuf {
    uint8_t* p = nullptr;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc((void**)&p, std::max<size_t>(n, 16), hipHostMallocDefault); }
};

constexpr size_t DEFAULT_CHUNK = (size_t)1 << 19;                  // bytes per channel and file (the header has the arenas this gives)

// one file's place in the lockstep
struct Run {
    long got = 0;                      // bytes per channel of the chunk in hand; 0: the file has ended (or never began)
    size_t carry = 0, carry_at = 0;    // frames no block has taken yet, and the frame they begin at in the encoder's buffer in use
    size_t l_have = 0, l_at = 0;       // frames the meter keeps, and the frame they begin at in the meter's buffer in use
    uint64_t l_first = 0, l_next = 0;  // the stream position of the first kept frame; the next sub-block to measure
    uint64_t done = 0;
};

int file_fail(int code, uint32_t f, const std::string& message) { return fail(code, "file " + std::to_string(f) + ": " + message); }

}  // namespace

#define STREAMS_HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, what); } while (0)

extern "C" int d2d_convert_streams_flac(d2d_engine* e, d2d_stream_io* io, uint32_t n, const d2d_streams_options* opt) {
    // every parameter is looked at before the first device call
    if (!opt || opt->struct_size < offsetof(d2d_streams_options, device_calls)) return fail(D2D_ERR_PARAM, "null options, or a struct_size that is not d2d_streams_options'");
    const bool has_counts = opt->struct_size >= sizeof(d2d_streams_options);
    uint64_t* const out_calls = has_counts ? opt->device_calls : nullptr;
    uint64_t* const out_chunks = has_counts ? opt->chunks : nullptr;
    const uint32_t bit_depth = opt->bit_depth, effort = opt->effort;
    if (!effort_ok(effort)) return fail(D2D_ERR_PARAM, EFFORT_MESSAGE);
    if (opt->flags & ~(uint32_t)(D2D_STREAMS_VERIFY | D2D_STREAMS_MD5)) return fail(D2D_ERR_PARAM, "unknown flags: D2D_STREAMS_VERIFY | D2D_STREAMS_MD5");
    if (!e) return fail(D2D_ERR_PARAM, "null engine");
    if (!io || n == 0) return fail(D2D_ERR_PARAM, "no files");
    if (d2d_tell(e, n - 1, nullptr, nullptr) != D2D_OK || d2d_tell(e, n, nullptr, nullptr) == D2D_OK) return fail(D2D_ERR_PARAM, "file count does not match the engine");
    if (!depth_ok(bit_depth)) return fail(D2D_ERR_PARAM, "FLAC holds 16, 20 or 24-bit integers (Invalid bit depth)");
    const size_t fb = d2d_frame_bytes(e), sb = sample_bytes(bit_depth);
    if (fb == 0 || fb % sb || fb / sb > 8) return fail(D2D_ERR_PARAM, "the engine's frames do not hold 1 to 8 channels of this bit depth");
    const uint32_t ch = (uint32_t)(fb / sb);
    const uint32_t in_ch = d2d_input_channels(e);      // the reads and uploads move whole INPUT frames: wider than the PCM's on a mixed or channel-subset engine
    const bool verify = (opt->flags & D2D_STREAMS_VERIFY) != 0, md5 = (opt->flags & D2D_STREAMS_MD5) != 0;
    uint32_t rate = 0;
    bool any_loud = false, any_tpeak = false, totals = true;
    uint64_t total = 0;
    for (uint32_t f = 0; f < n; ++f) {
        if (!io[f].read) return file_fail(D2D_ERR_PARAM, f, "null read callback");
        if (io[f].total_bytes_per_channel == 0) totals = false;
        total += io[f].total_bytes_per_channel;
        if (const d2d_loud* m = io[f].loud) {
            if (d2dloud::meter_channels(m) != ch) return file_fail(D2D_ERR_PARAM, f, "the meter was created for another channel count than the engine's");
            if (any_loud && d2dloud::meter_rate(m) != rate) return file_fail(D2D_ERR_PARAM, f, "the meter was created for another rate than the meters before it");
            rate = d2dloud::meter_rate(m); any_loud = true;
            any_tpeak = any_tpeak || d2dloud::meter_true_peak(m);
        }
    }
    const size_t chunk = opt->chunk_bytes_per_channel ? opt->chunk_bytes_per_channel : DEFAULT_CHUNK;
    uint64_t calls = 0, chunks = 0;
    auto counts = [&]() { if (out_calls) *out_calls = calls; if (out_chunks) *out_chunks = chunks; };
    counts();

    // the engine's device becomes this thread's current device (d2d_peak selects it and waits for the engine's pending work)
    double peak0 = 0.0;
    if (d2d_peak(e, 0, 0, &peak0) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
    for (uint32_t f = 0; f < n; ++f) {
        io[f].stats = d2d_flac_stream_stats{0, 0, 0, 0};
        if (verify) io[f].check = d2d_flac_check{0, 0, 0, 0xFFFFFFFFu, D2D_FLAC_BAD_NONE};
    }

    // per file, the single driver's sizes; one allocation of each kind, a 16-byte aligned slot per file
    size_t chunk_frames = 0;
    for (uint32_t f = 0; f < n; ++f) chunk_frames = std::max(chunk_frames, d2d_next_frames(e, f, chunk));
    chunk_frames += 64;
    const size_t cap_frames = chunk_frames + BS;
    const size_t in_slot = align16(chunk * in_ch), new_slot = align16(chunk_frames * fb), pcm_slot = align16(cap_frames * fb);
    const size_t out_slot = align16(d2d_flac_bound_bytes(ch, bit_depth, cap_frames, 1)), ws_slot = d2d_flac_workspace_bytes(ch, bit_depth, cap_frames, 1);
    const size_t S = rate / 10, l_cap = 3 * S + chunk_frames, l_rows = S ? l_cap / S + 2 : 0, loud_slot = align16(l_cap * fb);
    const size_t cells_slot = l_rows * ch * sizeof(d2d_loud_cell), peaks_slot = align16(l_rows * ch * sizeof(double));
    // (all device work goes to the null stream: the engine remembers the stream of its last call, d2d_flac_stream.cpp has the reason)
    const hipStream_t s = nullptr;
    PinBuf h_in[2], h_out, h_meta, h_cells, h_peaks, h_dig;
    DevBuf d_in, d_new, d_pcm[2], d_loud[2], d_out, d_ws, d_md5;
    STREAMS_HIP(h_in[0].alloc(n * in_slot), "hipHostMalloc"); STREAMS_HIP(h_in[1].alloc(n * in_slot), "hipHostMalloc");
    STREAMS_HIP(h_out.alloc(n * out_slot), "hipHostMalloc");
    // the records the kernels write for the host: results, checks, the pack's table
    const size_t res_at = 0, chk_at = align16(res_at + n * sizeof(d2d_flac_result)), off_at = align16(chk_at + n * sizeof(d2d_flac_check));
    STREAMS_HIP(h_meta.alloc(off_at + ((size_t)n + 1) * sizeof(uint64_t)), "hipHostMalloc");
    d2d_flac_result* const res = (d2d_flac_result*)(h_meta.p + res_at);
    d2d_flac_check* const chk = (d2d_flac_check*)(h_meta.p + chk_at);
    uint64_t* const offsets = (uint64_t*)(h_meta.p + off_at);
    STREAMS_HIP(d_in.alloc(n * in_slot), "hipMalloc"); STREAMS_HIP(d_new.alloc(n * new_slot), "hipMalloc");
    STREAMS_HIP(d_pcm[0].alloc(n * pcm_slot), "hipMalloc"); STREAMS_HIP(d_pcm[1].alloc(n * pcm_slot), "hipMalloc");
    STREAMS_HIP(d_out.alloc(n * out_slot), "hipMalloc"); STREAMS_HIP(d_ws.alloc(n * ws_slot), "hipMalloc");
    if (any_loud) {
        STREAMS_HIP(d_loud[0].alloc(n * loud_slot), "hipMalloc"); STREAMS_HIP(d_loud[1].alloc(n * loud_slot), "hipMalloc");
        STREAMS_HIP(h_cells.alloc(n * cells_slot), "hipHostMalloc");
    }
    if (any_tpeak) STREAMS_HIP(h_peaks.alloc(n * peaks_slot), "hipHostMalloc");
    if (md5) {
        STREAMS_HIP(d_md5.alloc(n * sizeof(d2d_flac_md5_state)), "hipMalloc"); STREAMS_HIP(h_dig.alloc(16 * (size_t)n), "hipHostMalloc");
        const int mrc = d2d_flac_md5_init_device(d_md5.p, n, s);
        ++calls;
        if (mrc != D2D_OK) return mrc;
    }

    std::vector<Run> run(n);
    std::vector<long> next(n);
    std::vector<d2d_file_io> tio(n);
    std::vector<d2d_flac_md5_io> mio(n);
    std::vector<d2d_loud_io> lio(n);
    std::vector<d2d_tpeak_io> pio(n);
    std::vector<d2d_flac_io> fio(n);
    std::vector<d2d_segment> seg;
    std::vector<d2d_pack_src> src(n);
    seg.reserve(4 * (size_t)n);
    int cur = 0, p_cur = 0, l_cur = 0;                              // the input arena, the encoder's and the meter's buffer in use
    uint64_t done = 0;
    bool any = false;
    for (uint32_t f = 0; f < n; ++f) {
        run[f].got = io[f].read(io[f].read_user, h_in[cur].p + f * in_slot, chunk);
        if (run[f].got < 0) return file_fail(D2D_ERR_IO, f, "read callback failed");
        any = any || run[f].got > 0;
    }
    while (any) {
        if (opt->cancel && *opt->cancel) return fail(D2D_ERR_CANCELLED, "Conversion cancelled");
        // upload and convert: every file's piece in its slot of the arena, one copy up to the last byte in use
        size_t in_bytes = 0;
        for (uint32_t f = 0; f < n; ++f) {
            const size_t L = (size_t)run[f].got;
            if (L > chunk) return file_fail(D2D_ERR_IO, f, "read callback returned more than it was asked for");
            if (L) in_bytes = f * in_slot + L * in_ch;
            tio[f] = d2d_file_io{};
            tio[f].dsd = d_in.p + f * in_slot; tio[f].bytes_per_channel = L; tio[f].pcm = d_new.p + f * new_slot; tio[f].pcm_capacity_bytes = new_slot;
        }
        STREAMS_HIP(hipMemcpyAsync(d_in.p, h_in[cur].p, in_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync");
        ++calls;
        if (d2d_translate_batch_device(e, tio.data(), n, s) != D2D_OK) return fail(D2D_ERR_DEVICE, d2d_last_error(e));
        ++calls;
        if (md5) {                                                  // the chunk's new frames, where the translate call left them
            for (uint32_t f = 0; f < n; ++f) mio[f] = d2d_flac_md5_io{tio[f].pcm, tio[f].frames_out};
            const int mrc = d2d_flac_md5_update_device(ch, bit_depth, mio.data(), n, d_md5.p, s);
            ++calls;
            if (mrc != D2D_OK) return mrc;
        }
        // what each file keeps goes to the front of the other buffer, its new frames behind it: encoder and meter alike
        seg.clear();
        for (uint32_t f = 0; f < n; ++f) {
            Run& r = run[f];
            if (r.got == 0) continue;
            const size_t nf = tio[f].frames_out;
            if (r.carry + nf > cap_frames) return file_fail(D2D_ERR_STATE, f, "a chunk produced more frames than planned");
            uint8_t* const to = d_pcm[p_cur ^ 1].p + f * pcm_slot;
            seg.push_back(d2d_segment{to, d_pcm[p_cur].p + f * pcm_slot + r.carry_at * fb, r.carry * fb});
            seg.push_back(d2d_segment{to + r.carry * fb, tio[f].pcm, nf * fb});
            if (io[f].loud) {
                if (r.l_have + nf > l_cap) return file_fail(D2D_ERR_STATE, f, "a chunk produced more frames than planned");
                uint8_t* const lto = d_loud[l_cur ^ 1].p + f * loud_slot;
                seg.push_back(d2d_segment{lto, d_loud[l_cur].p + f * loud_slot + r.l_at * fb, r.l_have * fb});
                seg.push_back(d2d_segment{lto + r.l_have * fb, tio[f].pcm, nf * fb});
                r.l_have += nf;
            }
        }
        p_cur ^= 1; l_cur ^= 1;
        {
            const int src_rc = d2d_segments_move_device(seg.data(), (uint32_t)seg.size(), s);
            ++calls;
            if (src_rc != D2D_OK) return src_rc;
        }
        // the next chunk is read while the GPU works: a file ends with this chunk if it has none
        for (uint32_t f = 0; f < n; ++f) {
            next[f] = 0;
            if (run[f].got == 0) continue;
            next[f] = io[f].read(io[f].read_user, h_in[cur ^ 1].p + f * in_slot, chunk);
            if (next[f] < 0) return file_fail(D2D_ERR_IO, f, "read callback failed");
        }
        if (any_loud) {                                             // every sub-block the chunk's frames complete
            for (uint32_t f = 0; f < n; ++f) {
                const Run& r = run[f];
                lio[f] = d2d_loud_io{}; pio[f] = d2d_tpeak_io{};
                lio[f].next_subblock = r.l_next; pio[f].next_subblock = r.l_next;
                if (r.got == 0 || !io[f].loud) continue;
                lio[f].pcm = d_loud[l_cur].p + f * loud_slot; lio[f].frames = r.l_have; lio[f].first_frame = r.l_first; lio[f].first_subblock = r.l_next;
                lio[f].final = next[f] == 0; lio[f].cells = (d2d_loud_cell*)(h_cells.p + f * cells_slot); lio[f].cells_capacity = l_rows * ch;
                if (!d2dloud::meter_true_peak(io[f].loud)) continue;
                pio[f].pcm = lio[f].pcm; pio[f].frames = lio[f].frames; pio[f].first_frame = lio[f].first_frame; pio[f].first_subblock = lio[f].first_subblock;
                pio[f].final = lio[f].final; pio[f].peaks = (double*)(h_peaks.p + f * peaks_slot); pio[f].peaks_capacity = l_rows * ch;
            }
            const int lrc = d2d_loud_measure_device(ch, bit_depth, rate, lio.data(), n, s);
            ++calls;
            if (lrc != D2D_OK) return lrc;
            if (any_tpeak) {
                const int prc = d2d_true_peak_measure_device(ch, bit_depth, rate, pio.data(), n, s);
                ++calls;
                if (prc != D2D_OK) return prc;
            }
        }
        for (uint32_t f = 0; f < n; ++f) {
            const Run& r = run[f];
            fio[f] = d2d_flac_io{};
            fio[f].pcm = d_pcm[p_cur].p + f * pcm_slot; fio[f].out = d_out.p + f * out_slot; fio[f].out_capacity_bytes = out_slot; fio[f].result = res + f;
            if (r.got == 0) continue;                               // 0 frames: no block, bytes_out = 0
            if (io[f].stats.blocks > 0xFFFFFFFFull) return file_fail(D2D_ERR_PARAM, f, "frame numbers are 31 bits");
            fio[f].frames = r.carry + tio[f].frames_out; fio[f].first_block = (uint32_t)io[f].stats.blocks; fio[f].final = next[f] == 0;
        }
        {
            const int rc = d2d_flac_encode_device_effort(ch, bit_depth, effort, fio.data(), n, d_ws.p, d_ws.bytes, s);
            ++calls;
            if (rc != D2D_OK) return rc;
        }
        if (verify) {
            const int vrc = d2d_flac_verify_device(ch, bit_depth, fio.data(), n, d_ws.p, d_ws.bytes, chk, s);
            ++calls;
            if (vrc != D2D_OK) return vrc;
        }
        // all files' frame bytes back to back into pinned memory, the lengths read where the encoder wrote them
        for (uint32_t f = 0; f < n; ++f)
            src[f] = d2d_pack_src{fio[f].out, &res[f].bytes_out, d2d_flac_bound_bytes(ch, bit_depth, fio[f].frames, fio[f].final)};
        {
            const int prc = d2d_segments_pack_device(src.data(), n, h_out.p, n * out_slot, offsets, s);
            ++calls;
            if (prc != D2D_OK) return prc;
        }
        STREAMS_HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
        ++calls; ++chunks;
        counts();
        if (offsets[n] == UINT64_MAX) return fail(D2D_ERR_STATE, "an encode call wrote more bytes than its bound");
        if (verify) {                                               // the records come with the results; a bad block keeps the chunk from every `write`
            for (uint32_t f = 0; f < n; ++f) {
                if (run[f].got == 0) continue;
                d2d_flac_check& c = io[f].check;
                c.samples_checked += chk[f].samples_checked; c.blocks_checked += chk[f].blocks_checked;
                if (chk[f].bad_blocks) {
                    c.first_bad_block = (uint32_t)io[f].stats.blocks + chk[f].first_bad_block; c.first_bad_reason = chk[f].first_bad_reason;
                    c.bad_blocks += chk[f].bad_blocks;
                    return file_fail(D2D_ERR_VERIFY, f, "FLAC verify failed: block " + std::to_string(c.first_bad_block) + " (" + reason_name(c.first_bad_reason) + ")");
                }
            }
        }
        any = false;
        for (uint32_t f = 0; f < n; ++f) {
            Run& r = run[f];
            if (r.got == 0) continue;
            if (d2d_loud* m = io[f].loud) {                         // the cells came with the result
                const int lrc = d2d_loud_add(m, lio[f].cells, lio[f].subblocks, lio[f].cells_out > lio[f].subblocks * ch);
                if (lrc != D2D_OK) return lrc;
                if (d2dloud::meter_true_peak(m)) {
                    const int prc = d2d_loud_add_true_peaks(m, pio[f].peaks, pio[f].subblocks, pio[f].peaks_out > pio[f].subblocks * ch);
                    if (prc != D2D_OK) return prc;
                }
                r.l_next = lio[f].next_subblock;
                const uint64_t keep_from = (r.l_next > 2 ? r.l_next - 2 : 0) * (uint64_t)S;     // the pre-roll of the next sub-block
                const size_t drop = (size_t)(keep_from - r.l_first);
                r.l_have -= drop; r.l_at = drop; r.l_first = keep_from;
            }
            const d2d_flac_result rr = res[f];
            if (rr.bytes_out != offsets[f + 1] - offsets[f]) return file_fail(D2D_ERR_STATE, f, "the packed length is not the encoder's");
            if (rr.bytes_out && io[f].write && io[f].write(io[f].write_user, h_out.p + offsets[f], (size_t)rr.bytes_out) != 0)
                return file_fail(D2D_ERR_IO, f, "write callback failed");
            d2d_flac_stream_stats& st = io[f].stats;
            if (fio[f].blocks) {
                st.min_frame_bytes = st.blocks ? std::min(st.min_frame_bytes, rr.min_frame_bytes) : rr.min_frame_bytes;
                st.max_frame_bytes = std::max(st.max_frame_bytes, rr.max_frame_bytes);
                st.blocks += fio[f].blocks;
                st.samples_per_channel += fio[f].frames_consumed;
            }
            r.carry = fio[f].frames - fio[f].frames_consumed; r.carry_at = fio[f].frames_consumed;
            done += (uint64_t)r.got;
            r.got = next[f];
            any = any || r.got > 0;
        }
        if (opt->progress && totals) {
            float pct = (float)(100.0 * (double)done / (double)total);
            if (pct >= 100.0f) pct = 99.99f;       // exactly 100 is reserved for the end
            opt->progress(opt->progress_user, pct);
        }
        cur ^= 1;
    }
    if (md5) {
        const int mrc = d2d_flac_md5_final_device(d_md5.p, n, h_dig.p, s);
        ++calls;
        if (mrc != D2D_OK) return mrc;
        STREAMS_HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
        ++calls;
        for (uint32_t f = 0; f < n; ++f) memcpy(io[f].md5, h_dig.p + 16 * (size_t)f, 16);
    }
    counts();
    if (opt->progress) opt->progress(opt->progress_user, 100.0f);
    return D2D_OK;
}
