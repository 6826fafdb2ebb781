/* dsd2dxd_amd.h -- C ABI of the MI355X-native DSD->PCM decimation engine.
 *
 * This is the drop-in boundary for ONE path of clone206/dsd2dxd: the conversion core that the
 * CLI reaches through the rdsd2pcm crate (the crate itself is an un-vendored submodule; the
 * surface below is reconstructed from its call sites in the reference).  The reference has no
 * FFI of its own for this path, so each entry point names the Rust item a binding would sit
 * behind.  INTEGRATION.md shows the `extern "C"` block and the Rdsd2Pcm shim a maintainer adds.
 *
 *   plain pointers and sizes only; caller-owned buffers; int status returns (0 = ok, <0 = error);
 *   one engine is used by one thread at a time (the reference builds one Rdsd2Pcm per Rayon
 *   worker, src/main.rs:280-300,361-394); different engines are fully independent.
 */
#ifndef DSD2DXD_AMD_H
#define DSD2DXD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_ABI_VERSION 11  /* 3: the table blob header names the table variant; 4: d2d_params.tap_bits; 5: d2d_params.debug_flags (was reserved0);
                             * 6: d2d_seek / d2d_tell / d2d_prime* and the two size queries (d2d_params unchanged);
                             * 7: the d2d_flac_* entry points and d2d_convert_stream_flac (d2d_params unchanged);
                             * 8: the FLAC efforts: d2d_flac_encode_device_effort / _host_effort, d2d_convert_stream_flac_effort (d2d_params unchanged);
                             * 9: FLAC effort 12, D2D_FLAC_EFFORT_LPC, through the same entry points (d2d_params unchanged);
                             * 10: verifying FLAC frames: d2d_flac_verify_device / _host, d2d_flac_decode_host, d2d_convert_stream_flac_verified,
                             *     d2d_flac_check, D2D_FLAC_BAD_*, D2D_ERR_VERIFY (d2d_params unchanged);
                             * 11: D2D_FILTER_EQUIRIPPLE_CASCADE, the two-stage definition of the 48 kHz multiples, as a value of
                             *     d2d_params.filter (d2d_params unchanged);
                             *     added under 11, nothing existing changed: the verify method, d2d_flac_verify_device_method / _host_method,
                             *     D2D_FLAC_VERIFY_*, d2d_flac_verify_stats; the d2d_flac_md5_* calls; the d2d_loud_* calls and
                             *     d2d_convert_stream_flac_loud; the d2d_true_peak_measure_* calls, d2d_tpeak_io and the meter's
                             *     d2d_loud_set_true_peak / _add_true_peaks / _true_peak; D2D_DBG_NO_DITHER_TABLE and d2d_dither_table_calls;
                             *     the d2d_segments_* calls, d2d_convert_streams_flac with d2d_stream_io / d2d_streams_options, and
                             *     d2d_loud_finish_album / d2d_loud_true_peak_album; the channel matrix: d2d_mix, d2d_create_mix, d2d_get_mix,
                             *     d2d_input_channels, d2d_mix_preset with D2D_MIX_LAYOUT_*, d2d_mix_frames_host, d2d_mix_error; the halved engine
                             *     (44.1 / 48 kHz): d2d_create_half, d2d_half_factor, d2d_half_taps, d2d_half_job, d2d_half_frames_host / _device,
                             *     d2d_half_error */

/* status codes */
enum {
    D2D_OK = 0,
    D2D_ERR_PARAM = -1,        /* invalid parameter value (message says which)                  */
    D2D_ERR_RATE = -2,         /* (dsd rate, output rate) combination not available             */
    D2D_ERR_FILTER = -3,       /* filter type not available for this rate combination           */
    D2D_ERR_DEVICE = -10,      /* no usable HIP device / HIP runtime error                      */
    D2D_ERR_CAPACITY = -20,    /* output buffer too small                                       */
    D2D_ERR_CANCELLED = -30,   /* cancel flag was raised (do_conversion's &AtomicBool)          */
    D2D_ERR_STATE = -40,       /* call sequence error                                           */
    D2D_ERR_IO = -50,          /* reader / sink callback failed                                 */
    D2D_ERR_VERIFY = -60       /* a FLAC frame did not verify (d2d_convert_stream_flac_verified) */
};

/* enum values mirror the reference's CLI characters so a binding can pass them through:
 *   FmtType     src/main.rs:183-191    Endianness src/main.rs:193-197
 *   FilterType  src/main.rs:199-205    DitherType src/main.rs:171-181 */
enum { D2D_FMT_INTERLEAVED = 0, D2D_FMT_PLANAR = 1 };
enum { D2D_LSB_FIRST = 0, D2D_MSB_FIRST = 1 };
enum { D2D_FILTER_EQUIRIPPLE = 'E', D2D_FILTER_XLD = 'X', D2D_FILTER_DSD2PCM = 'D', D2D_FILTER_CHEBYSHEV = 'C',
       /* extension (ABI 11; no counterpart in src/main.rs:199-205), "stages": the equiripple filter of the 48 kHz multiples (96000 /
        * 192000 / 384000) as the cascade the reference describes.  Stage A decimates the bits to 352.8 kHz and its samples are
        * rounded to the stage's own grid; stage B, a polyphase L/147 resampler, reads those samples.  'E' composes the two stages
        * into one polyphase filter on the bits wherever such a table ships (DSD64 and DSD128 to every 48 kHz multiple, DSD256 to
        * 192 and 384 kHz): no sample at 352.8 kHz, so none of the images that sampling folds down, and other bytes (DESIGN.md
        * section 0 has the differences).  Where 'E' is already two-stage (DSD256 to 96 kHz, DSD512) the two letters give the same
        * bytes.  44.1 kHz-family rates are refused with D2D_ERR_FILTER. */
       D2D_FILTER_EQUIRIPPLE_CASCADE = 'S' };
enum { D2D_DITHER_TPDF = 'T', D2D_DITHER_RECT = 'R', D2D_DITHER_FPD = 'F', D2D_DITHER_NONE = 'X',
       /* extension (no counterpart in src/main.rs:171-181): TPDF dither inside a second-order error-feedback
        * loop, noise transfer function (1 - z^-1)^2; integer depths, 44.1 kHz-family output rates.  The loop is a
        * recurrence through a rounding; it restarts from zero error at every output index that is a multiple of
        * 8192, so that those segments run side by side in a pass of their own. */
       D2D_DITHER_NOISE_SHAPED = 'N' };
/* which device kernel evaluates the FIR (same numbers either way) */
enum { D2D_KERNEL_AUTO = 0, D2D_KERNEL_LUT = 1, D2D_KERNEL_MFMA = 2 };
/* d2d_params.debug_flags (ABI 5): diagnostic dispatch switches.  0 = production dispatch; the library reads NO environment variable.
 * Each flag sends a conversion down an older kernel or route that produces the SAME bytes -- what the parity tests compare routes with
 * and what A/B measurements time; all are fixed when the engine is created. */
enum {
    D2D_DBG_NO_MX       = 1u << 0,   /* M = 32 / 64 / 128 stay off the fp6 x fp4 kernel (int8 pipelined kernel / older kernels)            */
    D2D_DBG_NO_GAINQ    = 1u << 1,   /* levels other than 0 dB, 20-bit and the float dither go back to the two-group / one-group kernels   */
    D2D_DBG_NO_COOP     = 1u << 2,   /* byte-interleaved input goes through the planar pre-pass instead of the kernels' own staging         */
    D2D_DBG_HOST_STAGED = 1u << 3,   /* host-pointer entry points stage through device buffers even when the GPU can address the memory   */
    D2D_DBG_NO_PIPE     = 1u << 4,   /* stereo conversions stay on the two-group kernel (no software-pipelined kernel)                    */
    D2D_DBG_MFMA_V1     = 1u << 5,   /* the one-group matrix-core kernel of round 1 for every decimation                                   */
    D2D_DBG_NO_INTQ     = 1u << 6,   /* the f64 epilogues instead of the all-integer requantisers                                           */
    D2D_DBG_NS_GENERAL  = 1u << 7,   /* the general noise-shaping kernel for stereo too                                                     */
    /* bits 8..15: waves per block of the matrix-core kernels (0 = their own choice)                                                        */
    D2D_DBG_TAPS32_2PASS = 1u << 16, /* tap_bits = 32: the two scratch passes and the combining pass where the one-pass kernel would serve  */
    D2D_DBG_NO_DITHER_TABLE = 1u << 17 /* every file hashes its own dither words inside the FIR kernel (no per-call table, d2d_dither_table_calls) */
};

/* The conversion parameters of Rdsd2Pcm::new (src/main.rs:325-342) that concern the hot path.
 * File/sink arguments (output type, out_dir, append_rate, base_dir, in_path) stay on the host
 * side of the binding. */
typedef struct d2d_params {
    uint32_t struct_size;   /* sizeof(d2d_params), for ABI growth                               */
    uint32_t dsd_rate;      /* 1,2,4,8 = DSD64..DSD512     `dsd_rate`     src/main.rs:94-96,334 */
    uint32_t output_rate;   /* Hz                          `output_rate`  src/main.rs:85-92,329 */
    uint32_t channels;      /*                             `channels`     src/main.rs:50-52,336 */
    uint32_t fmt;           /* D2D_FMT_*                   `fmt`          src/main.rs:332       */
    uint32_t endianness;    /* D2D_LSB_FIRST/MSB_FIRST     `endian`       src/main.rs:333       */
    uint32_t block_size;    /* bytes/channel/block, planar `block_size`   src/main.rs:75-78,335 */
    uint32_t filter;        /* D2D_FILTER_*                `filter`       src/main.rs:337       */
    uint32_t bit_depth;     /* 16,20,24 int; 32 float      `bit_depth`    src/main.rs:58-60,326 */
    uint32_t dither;        /* D2D_DITHER_*                `dither`       src/main.rs:331       */
    uint32_t kernel;        /* D2D_KERNEL_*                                                      */
    int32_t  device;        /* HIP device ordinal (Rayon workers can be pinned to GPUs)         */
    double   level_db;      /* volume in dB                `level_db`     src/main.rs:107-110   */
    uint64_t seed;          /* dither seed (counter-based generator)             */
    /* Channel subset (ABI 2; a 64-byte struct without these two means "all channels").  The engine
     * reads the `channels`-wide input but converts only channels [channel_first, channel_first +
     * channel_count) and its PCM frames are `channel_count` wide; filter state, dither and peaks of a
     * channel are the same as in a full conversion, so the ranks of a multi-GPU job can take a few
     * channels each of ONE multichannel stream (config 5) and the host interleaves their
     * frames.  channel_count = 0: all channels. */
    uint32_t channel_first;
    uint32_t channel_count;
    /* Tap grid (ABI 4; a 72-byte struct without these two means 24).  24: the taps are q * 2^-S with 24-bit q -- what every fast
     * kernel is built on.  32: the same designs on the grid q32 * 2^-(S+8) (filters/filter_tables.inc: half32), for callers who
     * need integer output closer to an f64-tap reference (DESIGN.md sections 0 and 4.5): the engine runs the FIR twice -- the 24-bit
     * table, then the small residual table q32 - 256 q -- and combines the two exact integer sums before level, dither and
     * requantisation; about three times the device time.  44.1k-family rates, dither T / R / F / X. */
    uint32_t tap_bits;
    uint32_t debug_flags;   /* D2D_DBG_* (ABI 5; 0 in production)                                    */
} d2d_params;

typedef struct d2d_engine d2d_engine;

/* ---- life cycle -------------------------------------------------------------------------- */

/* Replaces Rdsd2Pcm::new / ::from_container (src/main.rs:325-343,362-374): validates the
 * (filter, dsd rate, output rate, depth, dither) combination, picks the tap tables, builds the
 * device tables.  `n_files` independent files (each `channels` wide) share one engine so that a
 * whole batch goes to the GPU in one launch; n_files = 1 is the per-file object of the reference.
 * On failure *out is NULL and d2d_create_error() (thread-local) has the message the reference
 * stringifies at src/main.rs:343,374,393. */
int d2d_create(const d2d_params* params, uint32_t n_files, d2d_engine** out);
const char* d2d_create_error(void);
void d2d_destroy(d2d_engine* e);
/* Start all files again from the idle history (a fresh Rdsd2Pcm). */
int d2d_reset(d2d_engine* e);
/* Message for the last failing call on this engine (Box<dyn Error> text, src/main.rs:438). */
const char* d2d_last_error(const d2d_engine* e);

/* ---- sizes ------------------------------------------------------------------------------- */

/* Bytes of one interleaved PCM frame: channels * {2,3,3,4} for 16/20/24/32 (20-bit rides in a
 * 3-byte container: build_test_mono.sh:3-8). */
size_t d2d_frame_bytes(const d2d_engine* e);
/* Frames the next translate call on `file` will produce if it is fed `bytes_per_channel`. */
size_t d2d_next_frames(const d2d_engine* e, uint32_t file, size_t bytes_per_channel);

/* ---- the hot path ------------------------------------------------------------------------ */

/* The per-block translate step inside Rdsd2Pcm::do_conversion (src/main.rs:345,429): feed
 * `bytes_per_channel` more bytes per channel of file 0 (channels*bytes_per_channel bytes at `dsd`,
 * laid out as params.fmt/block_size say; README.md:9), get interleaved little-endian PCM frames.
 * FIR history, resampler history, dither counter and peak carry over to the next call.
 * Host pointers; returns when `pcm` is filled.  Buffers the GPU can address (hipHostMalloc / hipHostRegister, 16-byte
 * aligned) are read and written by the kernels in place; any other memory is staged through device buffers. */
int d2d_translate(d2d_engine* e, const uint8_t* dsd, size_t bytes_per_channel,
                  void* pcm, size_t pcm_capacity_bytes, size_t* frames_out);

/* WHAT A CALL MAY TOUCH (every translate and prime entry point; tests/test_gpu_containment.py pins it on every kernel route):
 *   1. A successful translate call writes exactly the bytes [0, frames_out * d2d_frame_bytes) of each file's `pcm` and no other
 *      byte of caller memory.  A file that yields no frames has no byte written.  pcm_capacity_bytes is only checked: the
 *      kernels never see it, so frames_out * d2d_frame_bytes is all a buffer has to hold, and files may lie back to back.
 *   2. d2d_prime and d2d_prime_batch_device write no PCM at all.
 *   3. The result depends only on the declared channels * bytes_per_channel input bytes of each file.
 *   4. A call that fails with D2D_ERR_CAPACITY or D2D_ERR_PARAM writes no PCM byte and leaves d2d_tell and d2d_peak of every file
 *      as they were; the engine goes on converting correctly.  (d2d_translate_batch_host checks every file's whole call --
 *      d2d_next_frames(e, f, bytes_per_channel) * d2d_frame_bytes against its capacity -- before it stages the first slice.) */

/* One file of a batch: device-resident input and output for the many-file path. */
typedef struct d2d_file_io {
    const void* dsd;            /* DEVICE pointer, 16-byte aligned                              */
    size_t      bytes_per_channel;
    void*       pcm;            /* DEVICE pointer, 16-byte aligned                              */
    size_t      pcm_capacity_bytes;
    size_t      frames_out;     /* written by the call                                          */
} d2d_file_io;

/* All `n_files` files of the engine advance by one call each, in ONE set of launches on
 * `hip_stream` (a hipStream_t, NULL = the null stream).  Asynchronous: returns once the work is
 * enqueued; io[i].frames_out is known at return.  This is the Rayon par_iter over files
 * (src/main.rs:280-300) turned into a grid dimension.  The engine's state (history, job table,
 * scratch) lives on the device: successive calls on one engine must be ordered on the device, i.e.
 * use one stream or order the streams with events. */
int d2d_translate_batch_device(d2d_engine* e, d2d_file_io* io, uint32_t n_files, void* hip_stream);

/* The same batch with HOST-resident buffers: `dsd` and `pcm` of every d2d_file_io are host pointers.
 * PINNED buffers (hipHostMalloc / hipHostRegister, 16-byte aligned) are addressed by the kernels
 * themselves: one set of launches reads the DSD and writes the frames over the link, so upload,
 * conversion and download overlap by construction and nothing is staged (bench shape: 90 GB/s over
 * the link both ways, `pcie_inclusive`).  Any other memory -- or D2D_DBG_HOST_STAGED, or a file of 2 GiB
 * per channel and more -- takes the pipeline: the batch is cut along time into slices of about
 * `slice_bytes_per_channel` (0 = 4 MiB; whole planar blocks), and upload, conversion and download
 * of consecutive slices run on three streams over double-buffered device staging (77 GB/s with
 * pinned buffers; pageable ones serialise).  Synchronous: returns when every `pcm` is filled;
 * io[i].frames_out is the total.  What the many-file path of a host that holds its files in RAM
 * calls; the reference's analogue is one Rayon worker per file reading,
 * converting and writing block by block (src/main.rs:280-300,345). */
int d2d_translate_batch_host(d2d_engine* e, d2d_file_io* io, uint32_t n_files, size_t slice_bytes_per_channel);

/* Rdsd2Pcm::check_level's result (src/bin/dsd_levels/main.rs:252-262): peak of |sample * gain|
 * seen so far.  Synchronises with the engine's pending work. */
int d2d_peak(d2d_engine* e, uint32_t file, uint32_t channel, double* peak_out);
int d2d_peak_dbfs(d2d_engine* e, uint32_t file, float* dbfs_out);

/* ---- time slices: start anywhere in a stream (ABI 6) -------------------------------------- */

/* A FIR output depends only on its own bit history, the dither generator is keyed by (seed, channel, absolute output
 * index) and the noise shaper restarts at every output index that is a multiple of 8192: an engine that knows its absolute
 * position and has seen a short halo produces the same bytes as one that converted the stream from its first byte.
 *
 * Below, F(p) is the number of frames an uninterrupted conversion has produced after p bytes per channel (no alignment
 * of p is needed).  THE GUARANTEE: for every p and every q <= max(0, p - d2d_preroll_bytes(e)), the sequence
 * d2d_seek(q), prime with the bytes [q, p), translate calls from p on yields byte for byte the frames F(p), F(p) + 1, ...
 * of the uninterrupted conversion, and the peak then read is the peak of exactly those frames.  N ranks can therefore cut
 * ONE stream along time (dsd2dxd_amd/shard.py: shard_time), each reading 1/N of the bytes plus the
 * halo, and a caller can convert an excerpt or resume an interrupted conversion without re-reading the file. */

/* Put `file` into the state of a fresh engine that stands at `bytes_per_channel`: idle bit history, zero stage-A
 * history, zero shaper errors, zero peaks; position, FIR and frame counters as after that many bytes.  Other files are
 * untouched; d2d_seek(e, f, 0) is d2d_reset for one file.  Synchronises with the engine's pending work, as d2d_reset. */
int d2d_seek(d2d_engine* e, uint32_t file, uint64_t bytes_per_channel);
/* Where `file` stands: bytes per channel consumed, and F of that = the index of the next frame.  Host state only; does
 * not synchronise.  Either pointer may be NULL. */
int d2d_tell(const d2d_engine* e, uint32_t file, uint64_t* bytes_per_channel, uint64_t* next_frame);
/* The halo of the guarantee above, in bytes per channel, from the engine's tables: window plus one decimation step for a
 * single filter; the carried history of a composed polyphase filter; stage A's window plus P + 1 stage-A outputs for the
 * 48k cascade.  Below 1 KiB for every shipped table.  A halved engine (d2d_create_half) adds the input of the NT - 1 sums
 * its decimator carries: about 1.5 to 6 KiB in all for its shapes. */
size_t d2d_preroll_bytes(const d2d_engine* e);
/* Noise-shaped dither ('N', integer depths) can only start where the shaper's state is known: at a frame index that is a
 * multiple of 8192.  This is the smallest A with F(k A) a multiple of 8192 for every k -- cut such streams at multiples
 * of it; 1 for every other engine.  After d2d_seek to a position > 0 or a prime, a translate call on that file whose
 * first frame index is not a multiple of 8192 fails with D2D_ERR_STATE and changes nothing (a call that produces no
 * frames for the file passes); one that starts on a multiple clears the condition. */
size_t d2d_slice_align_bytes(const d2d_engine* e);
/* d2d_translate's twin (host pointer, file 0): consumes the bytes exactly as d2d_translate would -- same layout rules --
 * and leaves position, bit history and stage-A history as it would, but produces NO frames and leaves the peaks
 * unchanged: only the kernels whose results carry over run (de-interleave pre-pass, stage A of the cascade, history
 * carry).  With profiling enabled its kernels are timed like a translate call's (d2d_profile_read_all: step time). */
int d2d_prime(d2d_engine* e, const uint8_t* dsd, size_t bytes_per_channel);
/* d2d_translate_batch_device's twin: same checks on `dsd` (16-byte aligned device pointer, below 2 GiB per call); `pcm`
 * and `pcm_capacity_bytes` are ignored and may be NULL / 0; frames_out is set to 0.  A file with bytes_per_channel = 0
 * is left as it is.  Asynchronous on `hip_stream`. */
int d2d_prime_batch_device(d2d_engine* e, d2d_file_io* io, uint32_t n_files, void* hip_stream);

/* ---- the channel matrix: fold a multichannel stream down inside the engine (added under ABI 11) ---- */

/* A mixed engine converts every one of params->channels input channels and emits frames of `out_channels` channels:
 * output o of a frame is sum_c coef[o * channels + c] / 32768 * (channel c's filtered sample), formed on the exact integer
 * FIR sums BEFORE level, dither and requantisation -- v_o = sum_c m[o][c] x_c is a 64-bit integer, y_o = v_o * 2^-(S+15)
 * exactly, and from y_o on channel o gets the arithmetic of every other path, its dither word keyed by (seed, OUTPUT
 * channel o, frame index).  DESIGN.md section 4.5b has the definition; 32768 times the identity gives the unmixed engine's
 * bytes and peaks.  Bounds (D2D_ERR_PARAM): 1 <= out_channels <= channels, |m| <= 2^17, every row's sum of |m| <= 2^21;
 * a row of zeros is allowed.  Refused with a message that names the reason: the noise-shaped dither, tap_bits = 32, a
 * channel subset (D2D_ERR_PARAM), and every configuration whose filter runs a second stage -- DSD256 -> 96 kHz, DSD512 ->
 * 48 kHz multiples, filter 'S' (D2D_ERR_FILTER).  d2d_frame_bytes, the capacity checks and d2d_peak (channel <
 * out_channels) follow out_channels; seek, prime, tell, the batch entry points and the whole-stream drivers work as on
 * any engine.  mix = NULL is d2d_create. */
typedef struct d2d_mix {
    uint32_t struct_size;      /* sizeof(d2d_mix) */
    uint32_t out_channels;     /* rows */
    const int32_t* coef;       /* out_channels x params->channels, row-major, Q15 */
} d2d_mix;
int d2d_create_mix(const d2d_params* params, const d2d_mix* mix, uint32_t n_files, d2d_engine** out);
/* The engine's mix: *out_channels = its rows (0: the engine does not mix) and, when coef is not NULL, the rows x channels
 * coefficients (capacity in int32; D2D_ERR_CAPACITY when they do not fit). */
int d2d_get_mix(const d2d_engine* e, uint32_t* out_channels, int32_t* coef, size_t capacity);
/* Channels of the engine's INPUT layout (params->channels): what a read callback fills per byte-per-channel, whatever the
 * width of the PCM frames (a mix, a channel subset). */
uint32_t d2d_input_channels(const d2d_engine* e);
/* The fold-down presets.  Columns in container order; the LFE is dropped; every row sums to at most 32768, so the fold
 * cannot clip where no single channel could.  target 2: rows Lo, Ro; target 1: one row, floor((Lo + Ro) / 2) per column.
 *   D2D_MIX_LAYOUT_5_1 (FL FR C LFE BL BR)  Lo 13573 0 9597 0 9597 0   Ro 0 13573 9597 0 0 9597
 *   D2D_MIX_LAYOUT_5_0 (FL FR C BL BR)      the same without the LFE column
 *   D2D_MIX_LAYOUT_QUAD (FL FR BL BR)       Lo 19195 0 13573 0         Ro 0 19195 0 13573
 *   D2D_MIX_LAYOUT_LRC (FL FR C), _LRC_LFE  Lo 19195 0 13573 (0)       Ro 0 19195 13573 (0)
 *   D2D_MIX_LAYOUT_STEREO (FL FR)           target 1 only: 16384 16384
 * D2D_MIX_LAYOUT_AUTO chooses by in_channels: 2 stereo, 3 L R C, 4 quad, 5 5.0, 6 5.1.  coef holds 2 * in_channels int32.
 * D2D_ERR_PARAM (message: d2d_mix_error) for a layout that does not have in_channels channels, no preset, or a bad target. */
enum { D2D_MIX_LAYOUT_AUTO = 0, D2D_MIX_LAYOUT_STEREO = 2, D2D_MIX_LAYOUT_LRC = 3, D2D_MIX_LAYOUT_QUAD = 4, D2D_MIX_LAYOUT_5_0 = 5,
       D2D_MIX_LAYOUT_5_1 = 6, D2D_MIX_LAYOUT_LRC_LFE = 7 };
int d2d_mix_preset(uint32_t in_channels, uint32_t layout, uint32_t target, int32_t* coef, uint32_t* out_channels);
/* The CPU twin of the mix pass, compiled from the kernel's own header; no device.  sums: channel c's exact integer FIR sums
 * of `frames` consecutive frames at sums[c * stride .. ], scale 2^-scale_bits; the first frame has index first_index (the
 * dither counter).  Writes `frames` interleaved frames of mix->out_channels samples to pcm and raises peaks[o] (when not
 * NULL; the caller zeroes them) to max |y_o * gain|.  bit_depth, dither (T / R / F / X), level_db and seed as in d2d_params. */
int d2d_mix_frames_host(const int32_t* sums, size_t stride, size_t frames, uint32_t in_channels, int32_t scale_bits, const d2d_mix* mix,
                        uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed, uint64_t first_index,
                        void* pcm, size_t pcm_capacity_bytes, double* peaks);
const char* d2d_mix_error(void);

/* ---- 44.1 and 48 kHz: an exact 2:1 decimator behind the FIR (added under ABI 11) ---- */

/* A halved engine converts to twice params->output_rate exactly as the 'N' dither's integer pass of that shape does (the
 * FIR kernels write every channel's exact integer sums x[i], scale 2^-S, into the scratch) and then low-pass filters and
 * decimates them by two in integer arithmetic.  With the NT taps q[j] at 2^-T of d2d_half_taps (symmetric, sum q = 2^T,
 * pass band to 0.22676 and stop band from 0.25 of the doubled rate) and x[i] = 0 for i < 0:
 *     v[k] = sum_j q[j] x[2k - j]        exact, 64-bit
 *     w[k] = (v[k] + 2^(T-1)) >> T       arithmetic shift: rounded to the scratch grid, ties towards +infinity
 *     y[k] = w[k] * 2^-S                 exact; from y on the arithmetic of every other path: peak = max |y * gain|, level,
 *                                        the dither word of (seed, channel, k), round half away from zero, clip, pack
 * DESIGN.md section 4.5c has the definition.  Frame k exists as soon as x[2k] does: after n sums a file has produced
 * (n + 1) >> 1 frames, and F(p) of the time-slice guarantee is that of the sums at p.  The filter's delay of (NT - 1) / 2
 * sums (about 2.2 ms) is NOT compensated.  d2d_next_frames, d2d_tell, d2d_frame_bytes, the capacity checks, d2d_peak,
 * d2d_reset, d2d_seek, d2d_prime*, d2d_translate*, the batch entry points and the whole-stream drivers follow the halved
 * frame sequence; d2d_preroll_bytes grows by the input of NT - 1 sums; d2d_get_info describes the FIR at the doubled rate.
 *
 * params->output_rate is the final rate: 44100 (DSD64 / DSD128 / DSD256; filter E, and X / C where they offer 88200) or
 * 48000 (DSD64 / DSD128, filter E); any other rate: D2D_ERR_RATE.  Refused with a message that names the reason: DSD512 and
 * DSD256 -> 48000, whose 96 kHz form runs a second stage with 64-bit sums (D2D_ERR_RATE); filters S and D (D2D_ERR_FILTER);
 * the noise-shaped dither, tap_bits = 32 and a channel subset (D2D_ERR_PARAM).  There is no mixed form.  d2d_create keeps
 * refusing 44100 and 48000. */
int d2d_create_half(const d2d_params* params, uint32_t n_files, d2d_engine** out);
/* 2 for an engine of d2d_create_half, 0 for every other engine */
uint32_t d2d_half_factor(const d2d_engine* e);
/* The decimator's table: *nt taps at 2^-*t; taps (capacity in int32) may be NULL to ask for the sizes alone;
 * D2D_ERR_CAPACITY when they do not fit. */
int d2d_half_taps(uint32_t* nt, uint32_t* t, int32_t* taps, size_t capacity);
/* The pass on its own.  One job is one file of a call: channel c's line at sums + c * stride holds the NT - 1 sums in front
 * of the call (zeros at the start of a stream) followed by its n new ones (stride >= NT - 1 + n); first_index is the absolute
 * index of the first new sum.  The frames k with first_index <= 2k < first_index + n are written to pcm, interleaved
 * (frames_out: how many), and peaks[c] (when not NULL; the caller zeroes them) is raised to max |y * gain|.  Channel c's
 * dither words are those of (seed, c, k).  bit_depth, dither (T / R / F / X), level_db and seed as in d2d_params;
 * scale_bits is S.  A job with n = 0 does nothing.  Errors: d2d_half_error. */
typedef struct d2d_half_job {
    const int32_t* sums;
    size_t stride;             /* int32 between the channels' lines */
    size_t n;                  /* new sums per channel */
    uint64_t first_index;
    void* pcm;
    size_t pcm_capacity_bytes;
    double* peaks;             /* `channels` doubles, or NULL */
    size_t frames_out;         /* written by the call */
} d2d_half_job;
/* the CPU twin of the kernel, compiled from the kernel's own header; no device */
int d2d_half_frames_host(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits,
                         uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed);
/* The same call on the current device: sums, pcm (16-byte aligned) and peaks are GPU-addressable, every job goes into one
 * launch on `hip_stream`, and the call returns once it has finished.  n below 2^31 per job. */
int d2d_half_frames_device(d2d_half_job* jobs, uint32_t n_jobs, uint32_t channels, int32_t scale_bits,
                           uint32_t bit_depth, uint32_t dither, double level_db, uint64_t seed, void* hip_stream);
const char* d2d_half_error(void);

/* ---- whole-stream driver ------------------------------------------------------------------ */

/* do_conversion(&cancel, progress) for callers that own the I/O (src/main.rs:345,429):
 * `read` fills at most `cap` bytes per channel worth of DSD (returning bytes per channel read,
 * 0 at end of stream, <0 on error), `write` consumes PCM bytes; `cancel` is polled between
 * chunks (the &AtomicBool of src/main.rs:38,429); `progress` receives a percentage and exactly
 * 100.0f last (ONE_HUNDRED_PERCENT, src/main.rs:417-418). `total_bytes_per_channel` may be 0
 * when unknown (stdin): then only the final 100.0f is reported. */
typedef long (*d2d_read_fn)(void* user, uint8_t* dst, size_t cap_bytes_per_channel);
typedef int (*d2d_write_fn)(void* user, const void* pcm, size_t bytes);
typedef void (*d2d_progress_fn)(void* user, float percent);
int d2d_convert_stream(d2d_engine* e, d2d_read_fn read, void* read_user,
                       d2d_write_fn write, void* write_user,
                       const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                       uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel);

/* ---- FLAC frames on the GPU (ABI 7) -------------------------------------------------------- */

/* The frames FlacSink writes (csrc/flac/flac_frame_enc.h is the definition), produced where the PCM already is: fixed block size
 * 4096, independent channels, fixed-order-2 prediction, one Rice partition per subframe (verbatim subframes for a last block of
 * 1 or 2 samples), 16 / 20 / 24 bits, at most 8 channels.  The device and the host entry produce the same bytes.  The encoder's
 * verbatim escape for residuals beyond 30 bits cannot fire at these depths (|s| <= 2^23 gives |r| <= 2^25), so it does not exist on
 * the GPU.  None of these entry points takes an engine; samples are the interleaved little-endian frames the translate calls write
 * (16-bit in 2 bytes, 24-bit in 3, 20-bit as the 3-byte container shifted right by 4).
 *
 * THE BOUND.  A frame of n samples per channel holds: a header of at most 13 bytes (2 sync/block-size-class, 1 block size and rate
 * codes, 1 channels and sample size, at most 6 for a 31-bit frame number, 2 for n - 1 when n != 4096, 1 CRC-8; counted as 4 + 6 + 2
 * + 1), `channels` subframes, zero bits up to a byte, and 2 bytes of CRC-16.  A subframe is 8 header bits, two warm-up samples of
 * `depth` bits, 11 bits of residual header and the Rice codes.  k is the smallest value with 2^k >= mean = floor(sum / (n - 2)), so
 * sum < (2^k + 1)(n - 2); with u_i <= 2 |r_i| the unary parts hold  sum(u_i >> k) <= 2 sum / 2^k < 2 (1 + 2^-k)(n - 2) <= 4 (n - 2)
 * zeros, and every code adds a stop bit and k <= 25 low bits: under 30 (n - 2) bits.  So
 *     subframe_bits(n)  <= 19 + 2 depth + 30 max(n - 2, 0)          (a verbatim subframe, n <= 2, is 8 + n depth)
 *     frame_bytes(n)    <= D2D_FLAC_FRAME_BOUND(n) = 15 + ceil(channels * (19 + 2 depth + 30 max(n - 2, 0)) / 8)
 *     d2d_flac_bound_bytes = floor(frames / 4096) * D2D_FLAC_FRAME_BOUND(4096) + (final and frames % 4096 ? D2D_FLAC_FRAME_BOUND(frames % 4096) : 0)
 * Host arithmetic, no device; 0 for parameters the encoders refuse.
 *
 * EFFORTS (ABI 8).  Everything above describes effort 0, which every entry point without `effort` in its name means.  Effort 1 is
 * the search that csrc/flac/flac_frame_enc.h defines: per subframe the fixed predictor order 0 .. 4 with the least exact cost at one
 * partition (the smallest order wins a tie), then the Rice partition order 0 .. pmax with the least exact cost (the smallest wins a
 * tie; pmax the largest p <= 6 with n % 2^p == 0 and (n >> p) >= 16), each partition's k by the rule above; for two channels the
 * least of independent, left/side, side/right and mid/side (ties in that order), the side channel one bit wider.  Frames of fewer
 * than 16 samples are the effort-0 frames.  THE BOUND DOES NOT CHANGE: (order 2, one partition) and the independent assignment are
 * always candidates and the costs are exact bit counts, so an effort-1 frame is never longer than the effort-0 frame of the same
 * samples; the argument for k (under 30 bits per residual) holds per partition, and |S| <= 2^24 gives |r_4| <= 2^28, so no escape
 * exists here either.  D2D_FLAC_FRAME_BOUND, d2d_flac_bound_bytes, d2d_flac_workspace_bytes and the slots serve every effort.
 *
 * Effort 12 (ABI 9; the value is the highest LPC order searched) adds linear predictors of order 4, 8 and 12 with 14-bit
 * coefficients to effort 1, per candidate signal, by rules 9 to 19 of csrc/flac/flac_frame_enc.h: an exact integer autocorrelation of
 * the windowed signal, one serial f64 routine from it to the quantised coefficients (csrc/flac/flac_lpc.h, the same source on the host
 * and on the GPU), exact costs.  A signal takes its LPC plan only where that is strictly cheaper than its effort-1 plan after both
 * partition searches, so an effort-12 frame is never longer than the effort-1 frame of the same samples and THE BOUND STANDS; every
 * residual stays below 2^30 in magnitude.  Frames of fewer than 64 samples are the effort-1 frames.  The values 2 .. 11 and everything
 * above 12 are unknown efforts. */
#define D2D_FLAC_BLOCK 4096u
enum { D2D_FLAC_EFFORT_FIXED2 = 0, D2D_FLAC_EFFORT_SEARCH = 1, D2D_FLAC_EFFORT_LPC = 12 };
size_t d2d_flac_bound_bytes(uint32_t channels, uint32_t bit_depth, size_t frames, int final);
/* Scratch one d2d_flac_encode_device call needs for one such file: a 4-byte size per block, rounded up to 16 bytes, and one slot of
 * D2D_FLAC_FRAME_BOUND(4096) bytes, rounded up to 16, per block.  A call over several files needs the sum. */
size_t d2d_flac_workspace_bytes(uint32_t channels, uint32_t bit_depth, size_t frames, int final);

typedef struct d2d_flac_result {
    uint64_t bytes_out;          /* frame bytes written to `out`                                 */
    uint32_t min_frame_bytes;    /* smallest and largest frame of the call (STREAMINFO); 0 and 0 */
    uint32_t max_frame_bytes;    /* when the call produced no block                              */
} d2d_flac_result;

typedef struct d2d_flac_io {
    const void* pcm;             /* DEVICE pointer, 16-byte aligned: `frames` interleaved frames */
    size_t      frames;
    uint32_t    first_block;     /* frame number of the first block                              */
    int32_t     final;           /* non-zero: the stream ends here, a short last block is coded  */
    void*       out;             /* DEVICE pointer, 16-byte aligned                              */
    size_t      out_capacity_bytes;   /* at least d2d_flac_bound_bytes(channels, depth, frames, final) */
    d2d_flac_result* result;     /* memory the GPU can address (device or pinned host); valid once the stream has synchronised */
    size_t      blocks;          /* written at return: floor(frames / 4096), plus the short one if final */
    size_t      frames_consumed; /* written at return: 4096 * blocks, or all frames if final     */
} d2d_flac_io;

/* Encodes the whole blocks of `n_files` independent files (and, where `final`, the short last one) in two launches on `hip_stream`
 * (a hipStream_t, NULL = the null stream): one workgroup per (file, block) writes its frame into a workspace slot, then a second
 * kernel packs each file's slots into its `out`.  No workgroup waits for another; the kernel boundary is the only ordering.
 * Asynchronous, like d2d_translate_batch_device: `blocks` and `frames_consumed` are known at return, the result records and the
 * frames once the stream has synchronised.  The caller keeps the remainder of under 4096 frames in front of its next PCM.  A file
 * with fewer than 4096 non-final frames yields 0 blocks and bytes_out = 0.  `workspace` is device memory, 16-byte aligned, of at
 * least the sum of d2d_flac_workspace_bytes over the files.  Runs on the current device.
 *
 * Checked on the host before anything is launched: bit_depth not 16 / 20 / 24, channels 0 or above 8, first_block + blocks above
 * 2^31, null or misaligned pointers -> D2D_ERR_PARAM; out_capacity_bytes below d2d_flac_bound_bytes, workspace too small ->
 * D2D_ERR_CAPACITY.  d2d_flac_error() (thread-local) has the message.
 *
 * WHAT A CALL MAY TOUCH (tests/test_gpu_flac.py pins it): a successful call writes exactly the bytes [0, bytes_out) of each file's
 * `out`, the result records, and bytes inside [workspace, workspace + workspace_bytes); no other byte.  A refused call writes
 * nothing, `blocks` and `frames_consumed` included. */
int d2d_flac_encode_device(uint32_t channels, uint32_t bit_depth, d2d_flac_io* io, uint32_t n_files,
                           void* workspace, size_t workspace_bytes, void* hip_stream);
/* The same call at a chosen effort (D2D_FLAC_EFFORT_*; d2d_flac_encode_device is effort 0).  An unknown effort -> D2D_ERR_PARAM,
 * checked with the rest before any device call.  Sizes, workspace and what a call may touch are those of effort 0. */
int d2d_flac_encode_device_effort(uint32_t channels, uint32_t bit_depth, uint32_t effort, d2d_flac_io* io, uint32_t n_files,
                                  void* workspace, size_t workspace_bytes, void* hip_stream);
const char* d2d_flac_error(void);

/* The same frames from HOST memory with the sink's own encoder, no device: the reference the GPU tests compare against.  `pcm`
 * needs no alignment.  Same checks and codes as the device entry (cap below the bound -> D2D_ERR_CAPACITY, nothing written). */
int d2d_flac_encode_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                         void* out, size_t out_capacity_bytes, d2d_flac_result* result, size_t* frames_consumed);
int d2d_flac_encode_host_effort(uint32_t channels, uint32_t bit_depth, uint32_t effort, const void* pcm, size_t frames, uint32_t first_block,
                                int final, void* out, size_t out_capacity_bytes, d2d_flac_result* result, size_t* frames_consumed);

/* d2d_convert_stream's twin: `write` receives FLAC frame bytes -- whole frames, in order -- instead of PCM, and `stats` what
 * STREAMINFO needs.  Built on the public calls: each chunk is uploaded, converted by d2d_translate_batch_device into device PCM
 * behind the carried remainder, encoded by d2d_flac_encode_device on the same stream, and only the frame bytes come back; `final` is
 * raised on the chunk after which `read` returns 0.  `bit_depth` (16 / 20 / 24) is passed explicitly because d2d_frame_bytes cannot
 * tell 20 from 24; it must be the engine's.  Single-file engines that convert all their channels (no channel subset); for planar
 * input chunk_bytes_per_channel must be a multiple of the block size (0 = 4 MiB).  Cancel and progress as in d2d_convert_stream,
 * exactly 100.0f last.  Single-buffered: upload, kernels and download of one chunk do not overlap the next chunk's.  On failure
 * d2d_flac_error() has the message (the engine's own where an engine call failed). */
typedef struct d2d_flac_stream_stats {
    uint64_t samples_per_channel;
    uint64_t blocks;
    uint32_t min_frame_bytes;    /* 0 and 0 for an empty stream */
    uint32_t max_frame_bytes;
} d2d_flac_stream_stats;
int d2d_convert_stream_flac(d2d_engine* e, uint32_t bit_depth, d2d_read_fn read, void* read_user,
                            d2d_write_fn write, void* write_user,
                            const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                            uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel, d2d_flac_stream_stats* stats);
int d2d_convert_stream_flac_effort(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* read_user,
                                   d2d_write_fn write, void* write_user,
                                   const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                                   uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel, d2d_flac_stream_stats* stats);

/* ---- Verifying the frames (ABI 10) ---------------------------------------------------------- */

/* The counterpart of `flac --verify`: every frame an encode call wrote is parsed, decoded and compared with the PCM it was made from,
 * where both still are.  One parser (csrc/flac/flac_parse.h, the same source on the host and in the kernel) reads what the encoders
 * here can write, a little generalised: verbatim subframes, fixed orders 0 .. 4, LPC orders 1 .. 32 with precision 1 .. 15 and shift
 * 0 .. 15 (the field is signed: 16 .. 31 are negative shifts, which FLAC forbids), Rice method `01` with partition orders 0 .. 15; block-size
 * codes of every kind, sample-rate code 0, independent channels up to 8 and the three stereo assignments, 16 / 20 / 24 bits, frame
 * numbers up to 31 bits.
 *
 * THE REASONS, in the order of the checks: the first check a block fails is its reason (the numbered rules at the head of
 * flac_parse.h).  CRC-16 comes before any subframe is parsed, so a frame damaged in storage or transit is CRC8 or CRC16, and the later
 * reasons are what an encoder bug would produce.  D2D_FLAC_BAD_SAMPLES is the last: the frame parses from its first bit to its last
 * and does not give the PCM.  The host and the device give the same record for the same bytes. */
enum { D2D_FLAC_BAD_NONE = 0,
       D2D_FLAC_BAD_SIZE,        /* size-table entry 0, or above the frame bound, or the frames of a file do not add up to bytes_out */
       D2D_FLAC_BAD_HEADER,      /* sync, reserved bits, or a field that is not this call's: n, channels, depth, frame number      */
       D2D_FLAC_BAD_CRC8, D2D_FLAC_BAD_CRC16,
       D2D_FLAC_BAD_UNSUPPORTED, /* valid FLAC that the encoders here never write: constant subframes, wasted bits, Rice method 00,
                                    escape partitions, the variable-block-size bit, sample-rate codes other than 0                */
       D2D_FLAC_BAD_SYNTAX,      /* reserved values, partition order impossible for n, bits run out                                */
       D2D_FLAC_BAD_LENGTH,      /* the subframes end, padding is not zero or the frame is not exactly its size                     */
       D2D_FLAC_BAD_SAMPLES };   /* decodes, and is not the PCM                                                                     */
typedef struct d2d_flac_check {
    uint64_t samples_checked;    /* samples per channel of the blocks that passed */
    uint32_t blocks_checked;     /* blocks looked at (= io.blocks)                */
    uint32_t bad_blocks;
    uint32_t first_bad_block;    /* index within the call; 0xFFFFFFFF: none       */
    uint32_t first_bad_reason;   /* D2D_FLAC_BAD_* of that block                  */
} d2d_flac_check;

/* Called after d2d_flac_encode_device[_effort] on the same `io` (blocks, frames_consumed and first_block as that call left them),
 * the same untouched `workspace` and the same stream.  Asynchronous: checks[f], one record per file in memory the GPU can address
 * (device or pinned), is valid once the stream has synchronised.  It checks the PACKED bytes [0, bytes_out) of each file's `out`
 * against `pcm`; bytes_out comes from the result record, the frame starts from the size table the encode call left at the front of
 * the file's workspace -- the one thing taken from the encoder, and checked: an entry that is 0, above D2D_FLAC_FRAME_BOUND(4096) or
 * reaching beyond bytes_out, and a last block that does not end at bytes_out, are D2D_FLAC_BAD_SIZE.  Two launches per sixteen files:
 * a status kernel decides each (file, block) -- one lane per frame, or by the METHOD below one workgroup per frame, which is what
 * this call runs -- and leaves a status word in the first word of the block's workspace slot, then one
 * workgroup per file turns the words into the record with plain stores.  No atomics, no waiting.
 *
 * Refused before anything is launched, with the codes of the encode call: a depth that is not 16 / 20 / 24, channels 0 or above 8, null
 * or misaligned pointers (checks: 8-byte aligned), first_block + blocks above 2^31 -> D2D_ERR_PARAM; a workspace too small ->
 * D2D_ERR_CAPACITY.
 *
 * WHAT A CALL MAY TOUCH (tests/test_gpu_flac_verify.py pins it): it writes the check records and bytes inside [workspace, workspace +
 * workspace_bytes) -- never `out`, `pcm` or the result records.  It reads pcm[0, frames_consumed * frame_bytes), out[0, bytes_out), the
 * size table and the result record.  A refused call writes nothing. */
int d2d_flac_verify_device(uint32_t channels, uint32_t bit_depth, const d2d_flac_io* io, uint32_t n_files,
                           void* workspace, size_t workspace_bytes, d2d_flac_check* checks, void* hip_stream);
/* Added under ABI 11 (no existing call or structure changed): the METHOD of the verify pass.  The record of a call does not depend on
 * it -- csrc/flac/flac_expect.h says why -- only its cost does, and the count of blocks each path decided.
 *   D2D_FLAC_VERIFY_SERIAL  the kernel described above: one lane per frame runs the parser, flac_parse.h, code after code.
 *   D2D_FLAC_VERIFY_COOP    one workgroup per frame.  The verifier holds the PCM, so it computes every residual, every code and every
 *                           bit position from the samples and COMPARES the frame's bits with them, all samples at once; only the
 *                           headers and one 5-bit parameter per Rice partition are read in order.  This path only ever says "good":
 *                           a frame it does not accept -- any mismatch, any field the encoders here never write -- is decided by the
 *                           serial parser in one lane of the same workgroup, so reasons and their order are SERIAL's.
 *   D2D_FLAC_VERIFY_AUTO    COOP.  d2d_flac_verify_device, d2d_flac_verify_host, d2d_convert_stream_flac_verified and the CLI's
 *                           --flac-verify are AUTO with stats = NULL.
 * An unknown method -> D2D_ERR_PARAM before anything is launched, nothing written.  `stats`, one per file in memory the GPU can address
 * (4-byte aligned) or NULL, is valid with the check records: fast_blocks counts the blocks the cooperative path accepted,
 * fallback_blocks those the serial parser decided (under SERIAL: all of them); the two add up to blocks_checked.  Everything else --
 * refusals, launches per sixteen files, what a call may touch (with `stats` beside the check records) -- is d2d_flac_verify_device's. */
enum { D2D_FLAC_VERIFY_AUTO = 0, D2D_FLAC_VERIFY_SERIAL = 1, D2D_FLAC_VERIFY_COOP = 2 };
typedef struct d2d_flac_verify_stats { uint32_t fast_blocks, fallback_blocks; } d2d_flac_verify_stats;
int d2d_flac_verify_device_method(uint32_t channels, uint32_t bit_depth, uint32_t method, const d2d_flac_io* io, uint32_t n_files,
                                  void* workspace, size_t workspace_bytes, d2d_flac_check* checks,
                                  d2d_flac_verify_stats* stats /* one per file, GPU-addressable, may be NULL */, void* hip_stream);
/* The CPU twin, no device: the same rules on one file in host memory; what the GPU tests compare against.  `out` holds bytes_out
 * bytes of frames made from the `frames` frames at `pcm` (first_block, final as at the encode call); `sizes` is the per-block size
 * array, or NULL: then the frames are walked by decoding (rule 10 of flac_parse.h: the CRC-16 is checked once the frame's end is
 * found, and a walk that loses the frame's end -- any reason but SAMPLES -- ends there: every later block is D2D_FLAC_BAD_SIZE).  Parameter checks and codes of
 * d2d_flac_encode_host. */
int d2d_flac_verify_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                         const void* out, size_t bytes_out, const uint32_t* sizes, d2d_flac_check* check);
/* ... at a chosen method (added under ABI 11): COOP runs the rule of flac_expect.h frame by frame and the serial parser on a frame it
 * does not accept, as the kernel does, so the agreement of the two methods can be tested without a GPU.  With sizes = NULL a frame's
 * end is only known by parsing: every block is then the serial parser's, under either method.  `stats` (one record, or NULL) as above. */
int d2d_flac_verify_host_method(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, uint32_t first_block, int final,
                                const void* out, size_t bytes_out, const uint32_t* sizes, d2d_flac_check* check, uint32_t method,
                                d2d_flac_verify_stats* stats);
/* A small FLAC decoder for what the sinks here write: a run of whole frames, numbered from first_block, into the packed little-endian
 * PCM the translate calls write (20-bit samples as the 3-byte container, the value shifted left by 4).  Every frame holds 4096
 * samples per channel but the last, which may hold fewer.  It writes exactly [0, *frames_out * frame_bytes) of `pcm` and stops at the
 * first bad frame: *frames_out counts the samples per channel up to there, `check` says why (blocks_checked counts the frames looked
 * at, the bad one included), and the return code is still D2D_OK.  pcm_capacity_bytes below what the frames' headers announce ->
 * D2D_ERR_CAPACITY, nothing written. */
int d2d_flac_decode_host(uint32_t channels, uint32_t bit_depth, const void* frames, size_t bytes, uint32_t first_block,
                         void* pcm, size_t pcm_capacity_bytes, size_t* frames_out, d2d_flac_check* check);
/* d2d_convert_stream_flac_effort with a verify pass: after each chunk's encode the verify is enqueued on the same stream and its
 * record read with the frame bytes.  `check` accumulates the whole stream (first_bad_block is a stream block index).  On a bad block
 * the call stops BEFORE that chunk is handed to `write` and returns D2D_ERR_VERIFY; d2d_flac_error() names the block and the reason.
 * With no bad block, `write` receives the bytes of the unverified call. */
int d2d_convert_stream_flac_verified(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* read_user,
                                     d2d_write_fn write, void* write_user,
                                     const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                                     uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel, d2d_flac_stream_stats* stats,
                                     d2d_flac_check* check);

/* ---- STREAMINFO's MD5 on the GPU (added under ABI 11: no existing call or structure changed) -- */

/* FLAC's STREAMINFO carries the MD5 of the unencoded audio.  The GPU path keeps the samples on the device, so the hash is taken there:
 * one chain per file, many files per call (MD5 is serial within a file; a batch is not).  OPT-IN: the calls above neither hash nor
 * change; a file written without these calls keeps 16 zero bytes, FLAC's "not computed".
 *
 * WHAT IS HASHED is what the host sink hashes: the interleaved samples as little-endian whole-byte integers.  16 and 24 bits: the
 * packed frames of the translate calls as they are.  20 bits: those calls keep the value shifted left by 4 in a 3-byte container;
 * each 3-byte sample is shifted right by 4 ARITHMETICALLY and emitted again as 3 little-endian bytes (csrc/flac/flac_md5.h: one
 * source for the host twin and the kernel).
 *
 * THE STATE is public, one record per file: a caller may keep, copy or build one.  `update` continues file i's hash with io[i].frames
 * frames; the record carries the bytes behind the last whole 64-byte block, so a call may end anywhere.  frames == 0 leaves the record
 * as it is; n_files == 0 launches nothing.  After an update the tail bytes at and behind tail_bytes are 0: for the same bytes the host
 * twin and the device call leave the same 96 bytes.  `final` pads and writes the digest and does NOT modify the state, so a caller may
 * ask for the digest so far; the bit length is the full 64-bit 8 * bytes.
 *
 * The device calls only enqueue on `hip_stream` (NULL = the null stream), like d2d_flac_encode_device, and take no engine: records and
 * digests are valid once the stream has synchronised.  One wave per file, all files of a call in one launch of up to 128 files
 * (their descriptors ride in the kernel arguments); a larger call is cut into launches of 128, which run one after another on the
 * stream: A CALL'S TIME GROWS WITH ceil(n_files / 128), not with n_files (while the device has a free SIMD per file).  A caller may
 * enqueue `update` on a stream of its own beside other work: it occupies one wave per file.
 *
 * Checked on the host before anything is launched: bit_depth not 16 / 20 / 24, channels 0 or above 8, a null `states` / `digests` /
 * `io`, states not 16-byte aligned, a pcm pointer that is not 16-byte aligned, or null with frames > 0 -> D2D_ERR_PARAM;
 * d2d_flac_error() has the message.
 *
 * WHAT A CALL MAY TOUCH (tests/test_gpu_flac_md5.py pins it): `init` and `update` write the n_files state records and nothing else;
 * `update` reads exactly the frames it is given; `final` writes 16 * n_files digest bytes and nothing else.  A refused call writes
 * nothing. */
typedef struct d2d_flac_md5_state {      /* 96 bytes; memory the GPU can address (device or pinned host), 16-byte aligned */
    uint32_t h[4];                       /* a, b, c, d */
    uint64_t bytes;                      /* bytes hashed so far, the tail included */
    uint32_t tail_bytes;                 /* 0 .. 63 (= bytes % 64) */
    uint32_t reserved;                   /* 0 */
    uint8_t  tail[64];                   /* the bytes behind the last whole 64-byte block */
} d2d_flac_md5_state;
typedef struct d2d_flac_md5_io {
    const void* pcm;                     /* DEVICE pointer, 16-byte aligned: `frames` interleaved frames as the translate calls pack them */
    size_t      frames;
} d2d_flac_md5_io;

void d2d_flac_md5_init_host(d2d_flac_md5_state* states, uint32_t n_files);
int  d2d_flac_md5_init_device(void* states, uint32_t n_files, void* hip_stream);
int  d2d_flac_md5_update_device(uint32_t channels, uint32_t bit_depth, const d2d_flac_md5_io* io, uint32_t n_files,
                                void* states, void* hip_stream);
int  d2d_flac_md5_final_device(const void* states, uint32_t n_files, void* digests /* 16 bytes per file, GPU-addressable */, void* hip_stream);
/* The CPU twins, no device: one file in host memory (`pcm` needs no alignment), the same checks and codes. */
int  d2d_flac_md5_update_host(uint32_t channels, uint32_t bit_depth, const void* pcm, size_t frames, d2d_flac_md5_state* state);
int  d2d_flac_md5_final_host(const d2d_flac_md5_state* state, uint8_t digest[16]);

/* d2d_convert_stream_flac_effort (check == NULL) or d2d_convert_stream_flac_verified (check != NULL) with one state record: after each
 * chunk's d2d_translate_batch_device the chunk's new frames are hashed on the same stream, and after the last chunk `md5` receives the
 * digest for STREAMINFO (an empty stream: the MD5 of no bytes, as the host sink writes for one).  `write` and `stats` receive what the
 * call without the hash gives them.  On any failure `md5` is left untouched.  The three stream calls above do not hash. */
int d2d_convert_stream_flac_md5(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* read_user,
                                d2d_write_fn write, void* write_user,
                                const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                                uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel, d2d_flac_stream_stats* stats,
                                d2d_flac_check* check /* NULL: not verified */, uint8_t md5[16]);

/* ---- Loudness where the PCM is (added under ABI 11: no existing call or structure changed) ---- */

/* Integrated loudness (ITU-R BS.1770 / EBU R128) and the sample peak of PCM that lies on the device, for ReplayGain tags.  OPT-IN: no call
 * above measures or changes.  The arithmetic is written once, in csrc/loud/loud_meter.h, for the host twin and the kernel: f64,
 * multiplications and additions only, never fused; the order of operations in that header is the definition.
 *
 * INPUT: the packed little-endian frames of the translate calls.  16 bits: v / 2^15.  20 and 24 bits: the 3-byte container value / 2^23.
 * 32 bits: the float widened to f64.  `rate` is a multiple of 10 in 8000 .. 1411200; a SUB-BLOCK is S = rate / 10 frames (100 ms).
 *
 * K-WEIGHTING: two biquads, transposed direct form II, whose ten f64 coefficients d2d_loud_coefficients derives on the host from the
 * analogue prototypes by the bilinear transform (at 48000 Hz: the standard's table).  out[] = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1
 * a2.  They travel to the device in the kernel arguments: libm decides no device result.
 *
 * A CELL is (energy, peak) of sub-block j and channel c: energy = the sum of y * y over the sub-block's frames in frame order, peak = the
 * largest |x| there.  THE ONE DEPARTURE FROM THE STANDARD: y over sub-block j is the filter's output when it is started from rest at
 * frame max(0, j - 2) * S, two sub-blocks of pre-roll, fixed.  Against one uninterrupted pass the energies differ by about 1e-13 relative;
 * in exchange every (file, sub-block, channel) is independent work -- one GPU lane each -- and no result depends on where a stream is cut
 * into calls.
 *
 * A CALL: `pcm` holds frames [first_frame, first_frame + frames) of the stream and must hold the pre-roll of the first sub-block asked
 * for: first_frame <= max(0, first_subblock - 2) * S, and first_frame == 0 when first_subblock < 2.  Every whole sub-block from
 * first_subblock on that the buffer holds is measured; a `final` call adds one more row of cells for a partial last sub-block (energy and
 * peak over the frames it has).  The cell of sub-block j, channel c is cells[(j - first_subblock) * channels + c].  Written at return, by
 * host arithmetic: subblocks (whole ones measured), cells_out (cells written: (subblocks + the partial row) * channels), next_subblock.
 * The caller keeps everything from frame max(0, next_subblock - 2) * S in front of its next PCM.  A file with frames == 0 is left
 * alone (its three counts are not written either); n_files == 0 launches nothing.
 *
 * d2d_loud_measure_device only enqueues on `hip_stream` (NULL = the null stream) and takes no engine: one launch covers up to 64 files
 * (their descriptors ride in the kernel arguments; a larger call is cut into launches of 64).  The counts are known at return, the cells
 * are valid once the stream has synchronised.  Checked on the host before anything is launched: bit_depth not 16 / 20 / 24 / 32, channels
 * 0 or above 8, a bad rate, a missing pre-roll, a null `io`, null or misaligned (16 bytes) pcm / cells -> D2D_ERR_PARAM; cells_capacity
 * below cells_out -> D2D_ERR_CAPACITY; d2d_flac_error() has the message.  A refused call writes nothing, the counts included.  A
 * successful call writes exactly cells_out cells per file and no other byte, and reads only the declared frames
 * (tests/test_gpu_loudness.py pins it).  d2d_loud_measure_host is the CPU twin for one file in host memory (no alignment needed): the
 * same checks, the same counts, the same cells bit for bit. */
typedef struct d2d_loud_cell { double energy, peak; } d2d_loud_cell;
typedef struct d2d_loud_io {
    const void*    pcm;                  /* DEVICE pointer, 16-byte aligned (the host twin: host memory, any alignment) */
    size_t         frames;               /* frames in pcm */
    uint64_t       first_frame;          /* the stream position of pcm's first frame */
    uint64_t       first_subblock;       /* the first sub-block to measure */
    int32_t        final;                /* non-zero: the stream ends with this buffer */
    uint32_t       reserved;             /* 0 */
    d2d_loud_cell* cells;                /* GPU-addressable (device or pinned host), 16-byte aligned */
    size_t         cells_capacity;       /* in cells */
    size_t         subblocks;            /* out: whole sub-blocks measured */
    size_t         cells_out;            /* out: cells written */
    uint64_t       next_subblock;        /* out: first_subblock + subblocks */
} d2d_loud_io;

int d2d_loud_coefficients(uint32_t rate, double out[10]);
int d2d_loud_measure_device(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_loud_io* io, uint32_t n_files, void* hip_stream);
int d2d_loud_measure_host(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_loud_io* io);

/* INTEGRATION, host only, plain f64, no device: the cells of one stream, in order, from either twin.  A 400 ms block b is sub-blocks
 * b .. b + 3 (hop: one sub-block); z_c = sum(energy) / (4 S); l_b = -0.691 + 10 log10(sum_c G_c z_c); blocks at or under -70 LUFS are
 * dropped, then blocks at or under (the loudness of the rest - 10 LU); `lufs` is the loudness of what remains.  `weights` NULL: G = 1 for
 * every channel, and 1, 1, 1, 0, 1.41, 1.41 for six (L R C LFE Ls Rs).  d2d_loud_add takes whole_subblocks rows of `channels` cells and,
 * with has_partial, one more row that contributes its peak only.  If no block lies above -70 LUFS, `valid` is 0, lufs is 0 and gain_db is
 * 0.  ReplayGain: gain_db = -18 - lufs; peak is the sample peak.  blocks_gated counts the blocks either gate dropped. */
typedef struct d2d_loud d2d_loud;
typedef struct d2d_loud_result {
    double   lufs, peak, gain_db;
    int32_t  valid;
    uint32_t reserved;
    uint64_t blocks_total, blocks_gated;
} d2d_loud_result;
int  d2d_loud_create(uint32_t channels, uint32_t rate, const double* weights /* NULL: the defaults */, d2d_loud** out);
int  d2d_loud_add(d2d_loud* h, const d2d_loud_cell* cells, size_t whole_subblocks, int has_partial);
int  d2d_loud_finish(const d2d_loud* h, d2d_loud_result* result);
void d2d_loud_destroy(d2d_loud* h);

/* TRUE PEAK, opt-in beside the cells above: the largest magnitude of the signal oversampled four times, which the sample peak of a
 * cell cannot see (a full-scale sine at fs/4 sampled at 45 degrees has the sample peak 0.70711 and reads 1.00956 here).  The definition
 * is csrc/loud/true_peak.h, one source for the host twin and the kernel: four phases of twelve taps, INTEGER coefficients over 8192, the
 * same at every rate; y_p(n) = sum over k = 0 .. 11 of C[p][k] * x(n - k) in f64, in that order, x = 0 before frame 0; the value is
 * |y| * 2^-13.  Every product is exact and for integer input every sum is too, so no result depends on how the frames are spread over
 * lanes or calls.  The TRUE PEAK OF A CELL (sub-block j, channel c) is the largest value over n in [j S, (j + 1) S) -- to the stream's end
 * for the partial row -- and the four phases.  An output belongs to the sub-block of its index n: the filter's delay of about six frames
 * is not compensated, and the eleven outputs behind a stream's last frame are dropped; hence the meter reports max(sample peak, largest
 * cell).  Input is finite: non-finite float samples give an unspecified value.
 *
 * A CALL is d2d_loud_measure_device's / _host's, with one difference: `pcm` must hold eleven frames of history in front of the first
 * sub-block asked for, not the pre-roll: first_frame <= max(0, first_subblock * S - 11).  A buffer that holds the loudness pre-roll
 * therefore always qualifies.  The value of sub-block j, channel c is peaks[(j - first_subblock) * channels + c].  Rows, the counts
 * (subblocks, peaks_out, next_subblock), `final`, the partial row, frames == 0 (left alone), launches of at most 64 files, the checks
 * before anything is launched or written, D2D_ERR_PARAM / D2D_ERR_CAPACITY and d2d_flac_error() are as there; `peaks` is 8-byte aligned
 * for the device call.  A successful call writes exactly peaks_out doubles per file and no other byte, and reads only the declared
 * frames (tests/test_gpu_true_peak.py pins it).  d2d_true_peak_measure_host gives the same doubles bit for bit. */
typedef struct d2d_tpeak_io {
    const void*    pcm;                  /* DEVICE pointer, 16-byte aligned (the host twin: host memory, any alignment) */
    size_t         frames;               /* frames in pcm */
    uint64_t       first_frame;          /* the stream position of pcm's first frame */
    uint64_t       first_subblock;       /* the first sub-block to measure */
    int32_t        final;                /* non-zero: the stream ends with this buffer */
    uint32_t       reserved;             /* 0 */
    double*        peaks;                /* GPU-addressable (device or pinned host), 8-byte aligned */
    size_t         peaks_capacity;       /* in doubles */
    size_t         subblocks;            /* out: whole sub-blocks measured */
    size_t         peaks_out;            /* out: doubles written */
    uint64_t       next_subblock;        /* out: first_subblock + subblocks */
} d2d_tpeak_io;
int d2d_true_peak_measure_device(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_tpeak_io* io, uint32_t n_files, void* hip_stream);
int d2d_true_peak_measure_host(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_tpeak_io* io);

/* The meter's side.  d2d_loud_set_true_peak switches a meter's true peak on or off BEFORE its first d2d_loud_add /
 * d2d_loud_add_true_peaks (afterwards: D2D_ERR_PARAM); off, a meter is what it was, and d2d_loud_finish and d2d_loud_result never
 * change.  d2d_loud_add_true_peaks takes whole_subblocks rows of `channels` doubles and, with has_partial, one more, in stream order,
 * independently of d2d_loud_add (a meter that was not switched on refuses: D2D_ERR_PARAM; rows behind the partial one: D2D_ERR_STATE).
 * d2d_loud_true_peak gives max(d2d_loud_result.peak, the largest double added); D2D_ERR_PARAM unless true-peak rows were added and
 * their whole and partial counts equal those given to d2d_loud_add.  d2d_convert_stream_flac_loud below, given a meter that was
 * switched on, also enqueues d2d_true_peak_measure_device on the same stream over the same carried PCM and feeds the doubles in. */
int d2d_loud_set_true_peak(d2d_loud* h, int on);
int d2d_loud_add_true_peaks(d2d_loud* h, const double* peaks, size_t whole_subblocks, int has_partial);
int d2d_loud_true_peak(const d2d_loud* h, double* out);

/* d2d_convert_stream_flac_md5 with `md5` allowed to be NULL (not hashed) and a meter behind it: after each chunk's
 * d2d_translate_batch_device the new whole sub-blocks are measured on the same stream (at the last chunk: the partial one too); the cells
 * come back with the frame bytes and go into `loud` (d2d_loud_add), which the caller created for the engine's channels and output rate
 * and finishes afterwards.  The PCM the driver carries from chunk to chunk grows from "under one FLAC block" to also cover the
 * pre-roll.  `write`, `stats`, `check` and `md5` receive what the calls without the meter give them.  The stream calls above do not
 * measure. */
int d2d_convert_stream_flac_loud(d2d_engine* e, uint32_t bit_depth, uint32_t effort, d2d_read_fn read, void* read_user,
                                 d2d_write_fn write, void* write_user,
                                 const volatile int* cancel, d2d_progress_fn progress, void* progress_user,
                                 uint64_t total_bytes_per_channel, size_t chunk_bytes_per_channel, d2d_flac_stream_stats* stats,
                                 d2d_flac_check* check /* NULL: not verified */, uint8_t md5[16] /* NULL: not hashed */, d2d_loud* loud);

/* ---- Many streams per call: an album as one batch (added under ABI 11: no existing call or structure changed) ---- */

/* A CHUNK'S BOOKKEEPING IN ONE LAUNCH.  A driver that carries PCM from chunk to chunk for many files has, per file and chunk, a handful
 * of device-to-device copies and one download of a length that only the device knows.  These two calls do all of them at once.  Both
 * follow d2d_loud_measure_device: the descriptors ride in the kernel arguments, a call larger than one launch takes (96 segments; 128
 * pack sources) is cut into launches that run in order on `hip_stream` (NULL = the null stream), the call only enqueues, takes no
 * engine, checks everything on the host before the first launch, and d2d_flac_error() has the message.
 *
 * d2d_segments_move_device copies seg[i].bytes bytes from seg[i].src to seg[i].dst for every i.  Both pointers are GPU-addressable
 * (device or pinned host); any alignment and any length, 0 included (such a segment's pointers are not looked at).  No dst range may
 * overlap a src range or another dst range of the same call (src ranges may overlap each other): checked on the host, D2D_ERR_PARAM,
 * nothing written; so are a null pointer and a range that wraps the address space.  A successful call writes exactly the dst ranges and
 * no other byte.  It reads the src ranges and, at most, the rest of the aligned 16-byte words that hold their first and last byte.
 *
 * d2d_segments_pack_device lays n variable-length segments back to back: segment k is *src[k].bytes bytes at src[k].base and lands at
 * dst + offsets[k], offsets[0] = 0, offsets[k + 1] = offsets[k] + *src[k].bytes, no padding.  `bytes` is GPU-addressable and is read ON
 * THE DEVICE when the launch runs (point it at d2d_flac_result::bytes_out: no synchronise lies between an encode and its download);
 * max_bytes is what the host knows about it.  `offsets` holds n + 1 entries, GPU-addressable, 8-byte aligned; `dst` is normally pinned
 * host memory, so one run of bytes for all files crosses the link, written by the kernel.  The host checks sum(max_bytes) <=
 * dst_capacity, else D2D_ERR_CAPACITY; null or misaligned pointers -> D2D_ERR_PARAM; nothing launched.  `dst` and `offsets` must not
 * overlap each other or a source (not checked: the lengths are not known).  If any *bytes_k > max_bytes_k on the device, nothing is
 * copied and every offsets[k], k = 0 .. n, is UINT64_MAX.  A successful call writes exactly offsets[n] bytes of dst, the table, and
 * nothing else.  n = 0 writes offsets[0] = 0.
 *
 * The _host twins do the same with memcpy on host memory (`bytes` read at the call): the same checks, the same bytes. */
typedef struct d2d_segment { void* dst; const void* src; size_t bytes; } d2d_segment;
typedef struct d2d_pack_src { const void* base; const uint64_t* bytes; size_t max_bytes; } d2d_pack_src;
int d2d_segments_move_device(const d2d_segment* seg, uint32_t n, void* hip_stream);
int d2d_segments_move_host(const d2d_segment* seg, uint32_t n);
int d2d_segments_pack_device(const d2d_pack_src* src, uint32_t n, void* dst, size_t dst_capacity, uint64_t* offsets, void* hip_stream);
int d2d_segments_pack_host(const d2d_pack_src* src, uint32_t n, void* dst, size_t dst_capacity, uint64_t* offsets);

/* THE BATCH DRIVER.  d2d_convert_streams_flac converts n_files streams in lockstep through ONE engine created with n_files files:
 * d2d_convert_stream_flac_loud for many streams.  Per chunk it reads each unfinished file's next piece into one pinned arena (one chunk
 * ahead, so that `final` is known), then enqueues on the null stream, in this order: one upload, one d2d_translate_batch_device, one
 * d2d_flac_md5_update_device (D2D_STREAMS_MD5), one d2d_segments_move_device (the carried PCM of encoder and meter and the new frames
 * behind it; the buffers alternate so that no segment overlaps), one d2d_loud_measure_device and one d2d_true_peak_measure_device (files
 * with a meter; with its true peak switched on), the encode, the verify (D2D_STREAMS_VERIFY), one d2d_segments_pack_device into pinned
 * memory; then ONE hipStreamSynchronize, then each file's `write` in file order from the calling thread.  The number of these calls per
 * chunk does not depend on n_files (*device_calls counts them and *chunks the chunks, where the pointers are given).  Files may have
 * different lengths: a file that has ended takes part with 0 bytes / 0 frames, which every device call leaves alone; a file with no
 * byte at all gets zero stats and no `write` call.  All files' meters, where given, are of the engine's channels and one rate.
 *
 * chunk_bytes_per_channel is per file; 0 = 512 KiB: with c the chunk, a 64-file stereo DSD64 -> 88.2 kHz 24-bit batch holds about
 * 380 c of pinned memory (two input arenas, the frame bytes) and 850 c of device memory (input, new PCM, two carried buffers each for
 * encoder and meter, frame bytes, workspace), 190 MiB and 425 MiB; DESIGN 4.6f has the sum.  For planar input a multiple of the block
 * size, as for the single-stream calls.
 *
 * THE GUARANTEE.  For every file the concatenation of the bytes given to `write` equals, byte for byte, what
 * d2d_convert_stream_flac_loud gives for that stream alone on an engine of one file with the same d2d_params, at any chunk size of
 * either call; `stats`, `check` and `md5` are equal, and the meter, once finished, gives the same d2d_loud_result and the same true peak
 * bit for bit.  It holds because a FIR output depends on its own file's bits only, the dither is keyed by (seed, channel, output index)
 * and not by file, FLAC blocks and loudness sub-blocks are cut by stream position and not by chunk, and MD5 is a chain per file.
 *
 * ERRORS.  The whole call ends at the first failing callback (D2D_ERR_IO), block that does not verify (D2D_ERR_VERIFY; no file's bytes
 * of that chunk reach `write`), raised cancel flag or device error; the message names the file index ("file 2: ...").  Parameter errors
 * are found before any device call.  `progress` receives the percentage of the summed total_bytes_per_channel (only when every file
 * states one) and exactly 100.0f last. */
enum { D2D_STREAMS_VERIFY = 1, D2D_STREAMS_MD5 = 2 };
typedef struct d2d_stream_io {
    d2d_read_fn read;  void* read_user;
    d2d_write_fn write; void* write_user;      /* write may be NULL */
    uint64_t total_bytes_per_channel;          /* 0: unknown */
    d2d_loud* loud;                            /* NULL: not measured; true peak as the meter says */
    d2d_flac_stream_stats stats;               /* out */
    d2d_flac_check check;                      /* out, when verifying */
    uint8_t md5[16];                           /* out, when hashing */
} d2d_stream_io;
typedef struct d2d_streams_options {
    uint32_t struct_size, bit_depth, effort, flags;   /* sizeof(d2d_streams_options); D2D_STREAMS_VERIFY | D2D_STREAMS_MD5 */
    size_t chunk_bytes_per_channel;                   /* per file; 0: the default */
    const volatile int* cancel;
    d2d_progress_fn progress; void* progress_user;
    uint64_t* device_calls;                           /* out, may be NULL: device calls the driver enqueued, synchronises included */
    uint64_t* chunks;                                 /* out, may be NULL: chunks it ran */
} d2d_streams_options;
int d2d_convert_streams_flac(d2d_engine* e, d2d_stream_io* io, uint32_t n_files, const d2d_streams_options* opt);

/* ALBUM LOUDNESS, host only.  d2d_loud_finish_album applies the two gates of d2d_loud_finish to the 400 ms blocks of all meters, taken
 * in meter order then block order (blocks do not span tracks); `peak` is the largest sample peak, gain_db = -18 - lufs, `valid` as
 * there.  Meters of different channels, rate or weights, a null meter or n = 0 -> D2D_ERR_PARAM.  With n = 1 it equals
 * d2d_loud_finish bit for bit.  d2d_loud_true_peak_album gives the largest d2d_loud_true_peak, under that call's conditions for each
 * meter. */
int d2d_loud_finish_album(const d2d_loud* const* meters, uint32_t n, d2d_loud_result* result);
int d2d_loud_true_peak_album(const d2d_loud* const* meters, uint32_t n, double* out);

/* ---- shared tables (multi-GPU)------------------------------------------------------------ */

/* The device filter tables as one opaque blob, so that rank 0 can broadcast them (RCCL) and
 * the other ranks adopt them instead of rebuilding: size query, export to / import from a
 * DEVICE buffer.  Import checks the blob's header against the engine's own configuration. */
size_t d2d_tables_bytes(const d2d_engine* e);
int d2d_tables_export_device(d2d_engine* e, void* dev_dst, size_t cap, void* hip_stream);
int d2d_tables_import_device(d2d_engine* e, const void* dev_src, size_t bytes, void* hip_stream);

/* ---- introspection ------------------------------------------------------------------------ */

typedef struct d2d_info {
    uint32_t decimation;     /* M of the integer decimator (stage A for the 48k family)        */
    uint32_t ntaps;
    uint32_t scale_bits;     /* taps are q * 2^-scale_bits                                      */
    uint32_t resamp_L, resamp_M, resamp_P;  /* 0 for the 44.1k family                           */
    uint32_t kernel;         /* D2D_KERNEL_LUT or D2D_KERNEL_MFMA actually in use               */
    uint32_t abi_version;
    char     filter_name[32];
} d2d_info;
int d2d_get_info(const d2d_engine* e, d2d_info* out);
/* Name of the device kernel that does the FIR, as rocprofv3 prints it (for bench/profiles). */
const char* d2d_kernel_name(const d2d_engine* e);
/* Added under ABI 11 (no existing call or structure changed).  A batch whose files all stand at the same output index asks every file
 * for the same dither words: such a call of the fp6 x fp4 kernel's dithered stereo frames at 0 dB (16, 24 bits) hashes them once, into an engine-owned table of
 * 4 bytes x channels x outputs of the call, and its files read them there (same bytes either way; D2D_DBG_NO_DITHER_TABLE keeps every
 * call off the table).  The number of calls so far that used the table; 0 for a null engine. */
uint64_t d2d_dither_table_calls(const d2d_engine* e);

/* ---- measurement ---------------------------------------------------------------------------- */

/* When enabled, every translate call brackets its FIR launch with hipEvents on the launch stream;
 * d2d_profile_read() synchronises, returns the summed FIR kernel time and launch count since the
 * last read, and clears them.  (The analogue of the library's own "DSP speed" log line that the
 * reference prints per file -- asset/progress.jpg.) */
int d2d_profile_enable(d2d_engine* e, int on);
int d2d_profile_read(d2d_engine* e, double* fir_ms_total, uint64_t* launches);
/* The same, plus the device time of EVERY kernel of the batch calls (de-interleave, FIR, noise-shaping
 * or stage-B resampler, history carry): a second event pair around the whole call.  The two figures are
 * the engine's "DSP speed" for single- and multi-kernel configurations. */
int d2d_profile_read_all(d2d_engine* e, double* fir_ms_total, double* step_ms_total, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* DSD2DXD_AMD_H */
