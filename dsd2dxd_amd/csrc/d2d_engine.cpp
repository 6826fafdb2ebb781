// d2d_engine.cpp -- host side of the engine and the C ABI of include/dsd2dxd_amd.h.
//
// One Engine is what the reference calls an Rdsd2Pcm (one per file, src/main.rs:325-342,361-394 there), widened to `n_files` files so
// that the Rayon par_iter over files (src/main.rs:280-300) becomes a grid dimension of one launch.  The engine owns, in HBM:
//   * the filter tables (nibble LUTs or int8 MFMA fragments; stage-B coefficients)
//   * per (file, channel): `keep` history bytes (ping-pong), the running peak, and for the 48k
//     cascade an f64 scratch line [P carried | stage-A outputs of this call]
// Every one of them is a Buf: it knows its size and frees itself, so the engine has no list of things to free and a buffer that failed to
// grow is empty, never stale.  Streams and events go in ~d2d_engine.
// What a launch needs and no call changes (the FIR, polyphase, resampler and noise-shaper arguments, the job count) is built once, at the end
// of d2d_create, into d2d_engine::launch.  A call (batch_call) is five steps joined by a CallPlan: plan (checks and counts, no HIP call),
// buffers, job table, launches, commit.
// No CPU fallback exists: without a HIP device d2d_create fails with D2D_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dsd2dxd_amd.h"
#include "d2d_filters.h"
#include "d2d_internal.h"
#include "d2d_launch.h"
#include "d2d_mfma.h"
#include "d2d_mx.h"
#include "d2d_px.h"
#include "d2d_route.h"
#include "d2d_sample.h"
#include "d2d_tables.h"
#include "mix/d2d_mix.h"
#include "half/d2d_half.h"

using namespace d2d;

namespace {

thread_local std::string g_create_error;

struct FileState {
    uint64_t pos = 0;    // bytes per channel consumed
    uint64_t nfir = 0;   // FIR outputs produced
    uint64_t nres = 0;   // stage-B outputs produced (48k family)
    bool ns_unknown = false;   // 'N' dither: the shaper's state is not the uninterrupted conversion's (after d2d_seek past 0 / a prime) until a
                               // translate call starts on a multiple of 8192, where the state is zero by definition
};

constexpr int JOB_SLOTS = 8;

// what a growing buffer waits for before its old memory goes (Buf::reserve)
inline auto wait_stream(hipStream_t s) { return [s] { return hipStreamSynchronize(s); }; }
inline auto wait_device() { return [] { return hipDeviceSynchronize(); }; }

// Device memory (Pinned: hipHostMalloc memory) that knows its byte size and frees itself.  Move-only.
template <class T, bool Pinned = false>
struct Buf {
    T* p = nullptr;
    size_t bytes = 0;

    Buf() = default;
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }     // (no copies: this declares them away)
    ~Buf() { release(); }
    operator T*() const { return p; }
    size_t count() const { return bytes / sizeof(T); }

    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; bytes = 0;
    }
    hipError_t alloc(size_t n) {
        release();
        const hipError_t r = Pinned ? hipHostMalloc((void**)&p, n, hipHostMallocDefault) : hipMalloc((void**)&p, n);
        if (r == hipSuccess) bytes = n; else p = nullptr;
        return r;
    }
    // Nothing when the buffer holds n bytes already.  Otherwise: sync() (whatever may still use the old memory), free, allocate n; the old
    // contents are gone, and so is the buffer when the allocation fails.
    template <class Sync>
    hipError_t reserve(size_t n, Sync sync) {
        if (n <= bytes) return hipSuccess;
        const hipError_t r = sync();
        return r != hipSuccess ? r : alloc(n);
    }
    // a create-time table
    hipError_t upload(const void* src, size_t n) {
        const hipError_t r = alloc(n);
        return r != hipSuccess ? r : hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    }
};

// Timing brackets of the measurement entry points: pairs of events, handed out one per bracket and summed by elapsed_ms.
struct EventPairs {
    typedef std::pair<hipEvent_t, hipEvent_t> Pair;
    std::vector<Pair> pool;
    size_t used = 0;

    ~EventPairs() { for (auto& pr : pool) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); } }
    // the next pair, its first event recorded on s; the caller records the second
    hipError_t open(hipStream_t s, Pair** out) {
        if (used == pool.size()) {
            Pair n{};
            hipError_t r = hipEventCreate(&n.first);
            if (r == hipSuccess) r = hipEventCreate(&n.second);
            if (r != hipSuccess) return r;
            pool.push_back(n);
        }
        *out = &pool[used++];
        return hipEventRecord((*out)->first, s);
    }
    // waits for every bracket handed out, sums them and hands them back
    hipError_t elapsed_ms(double* total) {
        *total = 0.0;
        for (size_t i = 0; i < used; ++i) {
            hipError_t r = hipEventSynchronize(pool[i].second);
            float ms = 0.f;
            if (r == hipSuccess) r = hipEventElapsedTime(&ms, pool[i].first, pool[i].second);
            if (r != hipSuccess) return r;
            *total += ms;
        }
        used = 0;
        return hipSuccess;
    }
};

// Everything a call's launches need that is fixed once d2d_create has made its choices.  batch_call copies what a launcher writes into and
// fills in what belongs to the call (the shaper's ping-pong state and grid, the cascade's f64 line).
struct LaunchState {
    FirLaunch fir;             // the main table, or the composed polyphase pass
    FirLaunch fir_lo;          // 32-bit taps in two passes: the residual table, on the second half of the job table and of the scratch
    FirLaunch fir_m2;          // MONO2: the pair kernel, on the half-call jobs behind the ordinary ones
    Rs2Args rs{};
    NoiseShapeArgs ns{};
    size_t njobs = 0;          // job rows per slot (32-bit taps: the second pass's jobs behind the first's; MONO2: the half-call jobs)
};

}  // namespace

struct d2d_engine {
    d2d_params p{};
    uint32_t n_files = 1;
    FilterChoice fc;
    int M = 0, Mb = 0, N = 0, Wb = 0, S = 0;
    uint32_t nstreams = 0;
    uint32_t Cin = 0;          // channels of the input layout
    uint32_t C = 0, c0 = 0;    // channels converted (streams per file; the width of the output frame unless the engine mixes) and the first of them
    // d2d_create_mix: Co rows x C columns of Q15 coefficients between the FIR sums and the requantiser (mix/d2d_mix.h).  The FIR pass is the 'N'
    // dither's integer pass of the same shape (plan_p, plan_epi: what the route and the launches are planned with; the caller's own parameters
    // on an unmixed engine), the mix pass makes the Co-wide frames (epi: its epilogue, channels = Co)
    std::vector<int32_t> mix;
    uint32_t Co = 0;           // width of the output frame: rows of the mix, or C
    bool mixed() const { return !mix.empty(); }
    d2d_params plan_p{};
    Epilogue plan_epi{};
    Buf<int32_t> d_mix;
    // d2d_create_half: p.output_rate is 44100 or 48000.  The FIR pass is the 'N' dither's integer pass of TWICE that rate (plan_p, fc, route: all
    // of the doubled rate), its sums go to the scratch behind the HALF_HIST carried ones (xs_hist), and the half pass (half/d2d_half.hip) makes the
    // frames: (n + 1) >> 1 of them after n sums
    bool half = false;
    uint64_t sums_at(uint64_t nfir, uint64_t nres) const { return fc.resamp ? nres : nfir; }          // the count the frames are numbered by ...
    uint64_t frames_at(uint64_t nfir, uint64_t nres) const { return half ? half_frames_after(sums_at(nfir, nres)) : sums_at(nfir, nres); }   // ... and the frames
    FirRoute route;            // which kernel, table layout and staging serve this engine (d2d_route.h: choose_route)
    MfmaLayout mfma{};
    mutable std::string kname; // d2d_kernel_name's answer before the first call
    std::string launched;      // the FIR kernel the last call really enqueued (d2d_last_launched_kernel)
    Epilogue epi{};
    std::string err;
    std::vector<FileState> files;

    // device
    Buf<uint8_t> d_fir_tables;
    Buf<uint8_t> d_resamp;
    Buf<uint8_t> d_hist[2]; int hist_cur = 0;
    Buf<double> d_peak;
    Buf<int32_t> d_scratch;               // stage-A integers, one line per stream (a multiple of 4 long), twice that with two-pass 32-bit taps
    bool noise_shape = false;             // 'N' dither: the FIR writes integers, a sequential pass requantises
    Buf<double> d_ns[2]; int ns_cur = 0;  // its state: two errors per stream, ping-pong between calls
    Buf<uint8_t> d_ns_dump;               // NoiseShapeArgs::dump
    Buf<double> d_ys;                     // 'N' on the 48k family: stage B's outputs as f64, one line per stream
    uint32_t xs_hist = 0;                 // samples carried in front of each scratch line (P of the resampler, else 0)
    Buf<StreamJob> d_jobs;
    Buf<StreamJob, true> h_jobs;          // pinned, JOB_SLOTS x launch.njobs
    hipEvent_t job_ev[JOB_SLOTS]{}; bool job_ev_used[JOB_SLOTS]{}; int job_slot = 0;
    hipStream_t own_stream = nullptr;     // used by the host-pointer entry points
    // d2d_translate_batch_host: upload / convert / download streams, their events, double-buffered staging
    hipStream_t hb_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t hb_ev[6] = {};
    Buf<uint8_t> hb_in[2], hb_out[2];
    hipStream_t last_stream = nullptr;
    // measurement
    bool profiling = false;
    EventPairs prof;                      // around the FIR launch
    EventPairs step;                      // around every kernel of a batch call
    // staging for d2d_translate (host pointers)
    Buf<uint8_t> d_in, d_out;
    // planar copies of byte-interleaved inputs (one slice per file), see d2d_deinterleave_kernel
    Buf<uint8_t> d_planar;
    // the dither words of a call whose files all start at the same output index, hashed once for all of them: [C][stride] (dither_table_serves)
    Buf<uint32_t> d_dither;
    uint64_t dither_table_calls = 0;      // calls that used it
    // route.fine (tap_bits = 32 in two passes): the second half of the scratch, of the job table and the residual table belong to the second pass
    std::vector<int32_t> lo_half;
    d2d_filter_def lo_def{};
    Buf<uint8_t> d_fir_tables_lo;
    // filter 'E', DSD64 / DSD128 -> 48k multiples and DSD256 -> 192 / 384 kHz: one polyphase pass over the bits (d2d_kernels_px.hip); fc.fir / fc.resamp
    // only count frames then
    const d2d_poly_def* poly = nullptr;
    // the two-kernel 48k path: DSD256 -> 96 kHz and DSD512 input, and every 48k multiple of an engine with filter 'S' (d2d_filters.h)
    bool cascade() const { return fc.resamp && !poly; }
    // route.mono2_pipe: calls the mono pair does not fit (odd sizes, very short ones) take the engine's ordinary mono kernel: same bytes either way
    bool mono2_ok() const { return route.mono2_pipe != PIPE_NONE; }
    Buf<uint8_t> d_fir_tables_m2;
    LaunchState launch;

    // strides of the per-stream / per-file buffers, in elements: what the buffers hold, never a second record of it
    size_t scratch_stride() const { return d_scratch.count() / ((size_t)nstreams * (route.fine ? 2u : 1u)); }
    size_t ys_stride() const { return d_ys.count() / nstreams; }
    size_t planar_stride() const { return d_planar.bytes / n_files; }

    ~d2d_engine() {
        for (hipEvent_t ev : job_ev) if (ev) hipEventDestroy(ev);
        for (hipEvent_t ev : hb_ev) if (ev) hipEventDestroy(ev);
        for (hipStream_t st : hb_stream) if (st) hipStreamDestroy(st);
        if (own_stream) hipStreamDestroy(own_stream);
    }

    int fail(int code, const std::string& m) { err = m; return code; }
    int hip_fail(hipError_t e, const char* what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return D2D_ERR_DEVICE;
    }
};

#define HIPCHK(e_, call)                                                  \
    do {                                                                  \
        hipError_t _r = (call);                                           \
        if (_r != hipSuccess) return (e_)->hip_fail(_r, #call);           \
    } while (0)

static uint64_t res_outputs_after(const d2d_engine* e, uint64_t nx) {
    if (!e->fc.resamp) return nx;
    if (nx == 0) return 0;
    return (nx * (uint64_t)e->fc.resamp->L - 1) / (uint64_t)e->fc.resamp->Mdn + 1;
}

static int validate(const d2d_params& p, std::string& err) {
    if (p.channels < 1 || p.channels > 64) { err = "Invalid channel count"; return D2D_ERR_PARAM; }
    if (p.bit_depth != 16 && p.bit_depth != 20 && p.bit_depth != 24 && p.bit_depth != 32) {
        err = "Invalid bit depth; must be 16, 20, 24 or 32"; return D2D_ERR_PARAM;
    }
    if (p.dither != 'T' && p.dither != 'R' && p.dither != 'F' && p.dither != 'X' && p.dither != 'N') {
        err = "Invalid dither type; must be T, R, F, or X"; return D2D_ERR_PARAM;   // src/main.rs:176-180
    }
    if (p.fmt != D2D_FMT_INTERLEAVED && p.fmt != D2D_FMT_PLANAR) {
        err = "Invalid format; must be I (interleaved) or P (planar)"; return D2D_ERR_PARAM;  // src/main.rs:187-190
    }
    if (p.endianness != D2D_LSB_FIRST && p.endianness != D2D_MSB_FIRST) { err = "Invalid endianness"; return D2D_ERR_PARAM; }
    if (p.fmt == D2D_FMT_PLANAR && p.block_size == 0) { err = "Invalid block size"; return D2D_ERR_PARAM; }
    if (p.kernel > D2D_KERNEL_MFMA) { err = "Invalid kernel selector"; return D2D_ERR_PARAM; }
    if (!isfinite(p.level_db)) { err = "Invalid level"; return D2D_ERR_PARAM; }
    if (p.channel_first >= p.channels || p.channel_count > p.channels - p.channel_first) { err = "Invalid channel subset"; return D2D_ERR_PARAM; }
    return D2D_OK;
}

// what d2d_create_mix refuses beyond d2d_create: the mix works on the exact int32 sums of whole files' channels
static int validate_mix(const d2d_params& p, const std::vector<int32_t>& m, uint32_t rows, std::string& err) {
    if (const char* why = mix_check(p.channels, rows, m.data())) { err = why; return D2D_ERR_PARAM; }
    if (p.dither == 'N') { err = "a mix does not combine with the noise-shaped dither; use T, R, F or X"; return D2D_ERR_PARAM; }
    if (p.tap_bits == 32) { err = "a mix does not combine with 32-bit taps"; return D2D_ERR_PARAM; }
    if (p.channel_first != 0 || (p.channel_count != 0 && p.channel_count != p.channels)) {
        err = "a mix does not combine with a channel subset: give the subset as rows of the mix"; return D2D_ERR_PARAM;
    }
    return D2D_OK;
}

// what d2d_create_half refuses beyond d2d_create, before the filter choice: the decimator reads exact int32 sums of whole files' channels and
// its frames go straight to the requantiser
static int validate_half(const d2d_params& p, std::string& err) {
    if (p.output_rate != 44100 && p.output_rate != 48000) { err = "Invalid output rate; a halved engine makes 44100 or 48000"; return D2D_ERR_RATE; }
    if (p.dsd_rate != 1 && p.dsd_rate != 2 && p.dsd_rate != 4 && p.dsd_rate != 8) { err = "Invalid DSD rate; must be 1, 2, 4 or 8"; return D2D_ERR_PARAM; }
    if (p.dsd_rate == 8) { err = "44100 / 48000 output: DSD512 input has no 88200 / 96000 form to halve"; return D2D_ERR_RATE; }
    if (p.dsd_rate == 4 && p.output_rate == 48000) {
        err = "48000 output needs DSD64 or DSD128 input: DSD256 -> 96000 runs a second stage, whose sums are not 32-bit integers"; return D2D_ERR_RATE;
    }
    if (p.filter == 'S') { err = "44100 / 48000 output: the two-stage equiripple filter's sums are not 32-bit integers; use filter E"; return D2D_ERR_FILTER; }
    if (p.filter == 'D') { err = "44100 / 48000 output: the dsd2pcm filter has no 88200 form to halve (DSD64 input and 352800 output only)"; return D2D_ERR_FILTER; }
    if (p.dither == 'N') { err = "44100 / 48000 output does not combine with the noise-shaped dither; use T, R, F or X"; return D2D_ERR_PARAM; }
    if (p.tap_bits == 32) { err = "44100 / 48000 output does not combine with 32-bit taps"; return D2D_ERR_PARAM; }
    if (p.channel_first != 0 || (p.channel_count != 0 && p.channel_count != p.channels)) {
        err = "44100 / 48000 output does not combine with a channel subset"; return D2D_ERR_PARAM;
    }
    return D2D_OK;
}

// what a stream that has not started yet holds as history
static uint8_t idle_byte(const d2d_engine* e) { return e->p.endianness == D2D_MSB_FIRST ? IDLE_BYTE : (uint8_t)0x96; }  // 0x69 bit-reversed

// The fills of create, d2d_reset and d2d_seek are null-stream hipMemsets.  The next call runs on a hipStreamNonBlocking stream (own_stream, or
// a caller's), which the null stream does not order, and a hipMemset of device memory may return before the fill has run: every path that
// fills ends here, so that the fills are ordered before whatever stream the next call uses.
static int fills_done(d2d_engine* e) {
    HIPCHK(e, hipDeviceSynchronize());
    return D2D_OK;
}

static int reset_state(d2d_engine* e) {
    HIPCHK(e, hipSetDevice(e->p.device));
    for (int b = 0; b < 2; ++b) HIPCHK(e, hipMemset(e->d_hist[b], idle_byte(e), e->d_hist[b].bytes));
    HIPCHK(e, hipMemset(e->d_peak, 0, e->d_peak.bytes));
    if (e->d_scratch) HIPCHK(e, hipMemset(e->d_scratch, 0, e->d_scratch.bytes));
    for (int i = 0; i < 2; ++i) if (e->d_ns[i]) HIPCHK(e, hipMemset(e->d_ns[i], 0, e->d_ns[i].bytes));
    for (auto& f : e->files) f = FileState{};
    e->hist_cur = 0;
    return fills_done(e);
}

// one file back to the device state of a fresh engine, in both ping-pong buffers; the other files' rows stay
static int clear_file_state(d2d_engine* e, uint32_t file) {
    const size_t s0 = (size_t)file * e->C;
    for (int b = 0; b < 2; ++b) HIPCHK(e, hipMemset(e->d_hist[b] + s0 * e->route.keep, idle_byte(e), (size_t)e->C * e->route.keep));
    HIPCHK(e, hipMemset(e->d_peak + s0, 0, sizeof(double) * e->C));
    if (e->d_scratch && e->xs_hist)     // the stage-A history in front of each of the file's scratch lines
        HIPCHK(e, hipMemset2D(e->d_scratch + s0 * e->scratch_stride(), e->scratch_stride() * sizeof(int32_t), 0, (size_t)e->xs_hist * sizeof(int32_t), e->C));
    for (int i = 0; i < 2; ++i) if (e->d_ns[i]) HIPCHK(e, hipMemset(e->d_ns[i] + 2 * s0, 0, sizeof(double) * 2 * e->C));
    return D2D_OK;
}

// d2d_engine::launch, once the route is chosen and every table and the job table exist
static void build_launch_state(d2d_engine* e) {
    LaunchState& l = e->launch;
    l.fir = fir_launch(e->plan_p, e->fc, e->plan_epi, e->route, PASS_MAIN);
    l.fir.bind(e->d_jobs, e->d_fir_tables);
    if (e->route.fine) {
        l.fir_lo = fir_launch(e->plan_p, e->fc, e->plan_epi, e->route, PASS_LO, &e->lo_def);
        l.fir_lo.bind(e->d_jobs + e->nstreams, e->d_fir_tables_lo);
    }
    if (e->mono2_ok()) {
        l.fir_m2 = fir_launch(e->plan_p, e->fc, e->plan_epi, e->route, PASS_MONO2);
        l.fir_m2.bind(e->d_jobs + e->nstreams, e->d_fir_tables_m2);
    }
    l.rs.jobs = e->d_jobs; l.rs.tables = e->d_resamp;
    l.rs.S = e->S; l.rs.epi = e->epi;
    NoiseShapeArgs& ns = l.ns;
    ns.jobs = e->d_jobs; ns.dump = e->d_ns_dump;
    ns.scale_bits = e->poly ? e->poly->S : e->S; ns.nstreams = e->nstreams; ns.epi = e->epi;
    ns.res = e->cascade() ? 1u : 0u;
    // the all-integer loop: the largest |y * 2^S| any output can reach (composed polyphase: its heaviest phase) leaves room for a few LSB
    const uint64_t sa = e->poly ? max_phase_sum_abs(*e->poly) : sum_abs_q(*e->fc.fir);
    ns.intq = (!(e->p.debug_flags & D2D_DBG_NO_INTQ) && sa + (1ull << 24) < (1ull << 31)) ? 1u : 0u;
    ns.general = (e->p.debug_flags & D2D_DBG_NS_GENERAL) ? 1u : 0u;
}

// d2d_create after the parameters are copied: every choice, table and buffer.  Errors go to e->err.
static int init_engine(d2d_engine* e) {
    int rc = validate(e->p, e->err);
    if (rc == D2D_OK && e->mixed()) rc = validate_mix(e->p, e->mix, e->Co, e->err);
    if (rc == D2D_OK && e->half) rc = validate_half(e->p, e->err);
    if (rc != D2D_OK) return rc;
    e->plan_p = e->half ? half_fir_params(e->p) : e->mixed() ? mix_fir_params(e->p) : e->p;
    rc = choose_filters(e->plan_p, e->fc, e->err);        // (plan_p differs from p in the rate only for a halved engine: the doubled one)
    // a mix reads exact int32 sums: a configuration whose filter choice has a stage B (DSD256 -> 96 kHz, DSD512 -> 48 kHz multiples, filter 'S')
    // has 64-bit ones
    if (rc == D2D_OK && e->mixed() && e->fc.resamp && !e->fc.poly)
        return e->fail(D2D_ERR_FILTER, "a mix needs a single-pass filter: this configuration runs a second stage (DSD256 -> 96 kHz, DSD512 -> 48 kHz "
                                       "multiples, filter S), whose sums are not 32-bit integers");
    if (rc == D2D_OK && e->half && e->fc.resamp && !e->fc.poly)
        return e->fail(D2D_ERR_RATE, "44100 / 48000 output needs a single-pass filter at the doubled rate: this one runs a second stage");
    if (rc == D2D_OK) rc = choose_route(e->plan_p, e->fc, e->route, e->err);
    if (rc != D2D_OK) return rc;
    const d2d_filter_def& f = *e->fc.fir;
    e->M = f.M; e->Mb = f.M / 8; e->N = f.ntaps; e->Wb = f.ntaps / 8; e->S = f.S;
    e->Cin = e->p.channels;
    e->epi = epilogue_of(e->p);
    e->plan_epi = epilogue_of(e->plan_p);
    e->C = e->epi.channels;
    if (e->mixed()) e->epi.channels = e->Co; else e->Co = e->C;
    e->c0 = e->p.channel_first;
    e->nstreams = e->n_files * e->C;
    e->files.resize(e->n_files);
    e->noise_shape = e->epi.dither == 'N';
    e->poly = e->fc.poly;
    e->mfma = mfma_layout(e->M, e->N);
    const FirRoute& r = e->route;

    // ---- device side: fail loudly when there is no GPU ----
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev <= 0)
        return e->fail(D2D_ERR_DEVICE, std::string("no HIP device available (") + (he != hipSuccess ? hipGetErrorString(he) : "device count 0") +
                                           "); this engine has no CPU path");
    if (e->p.device < 0 || e->p.device >= ndev) return e->fail(D2D_ERR_DEVICE, "Invalid device ordinal");
    HIPCHK(e, hipSetDevice(e->p.device));
    HIPCHK(e, hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    // ---- the tables the route names ----
    const bool msb = e->p.endianness == D2D_MSB_FIRST;
    if (e->poly) {
        if (r.poly_plain) {
            HIPCHK(e, e->d_fir_tables.upload(e->poly->q, (size_t)e->poly->Lp * e->poly->NP * sizeof(int32_t)));
        } else {
            const std::vector<int8_t> t = build_px_tables(*e->poly);
            HIPCHK(e, e->d_fir_tables.upload(t.data(), t.size()));
        }
    } else if (r.kernel == D2D_KERNEL_LUT) {
        const std::vector<double> t = build_lut_tables(f, e->Mb, msb);
        HIPCHK(e, e->d_fir_tables.upload(t.data(), t.size() * sizeof(double)));
    } else {
        const std::vector<int8_t> t = build_fir_table(f, r.mfma_pipe, r.mfma_v2, e->mfma, msb, r.taps32);
        HIPCHK(e, e->d_fir_tables.upload(t.data(), t.size()));
    }
    if (r.fine) {      // the residual table goes through the same builders
        e->lo_def = residual_def(f, e->lo_half);
        if (r.kernel == D2D_KERNEL_LUT) {
            const std::vector<double> tl = build_lut_tables(e->lo_def, e->Mb, msb);
            HIPCHK(e, e->d_fir_tables_lo.upload(tl.data(), tl.size() * sizeof(double)));
        } else {
            const std::vector<int8_t> tl = build_fir_table(e->lo_def, r.mfma_pipe_lo, r.mfma_v2, e->mfma, msb, false);
            HIPCHK(e, e->d_fir_tables_lo.upload(tl.data(), tl.size()));
        }
    }
    if (e->mono2_ok()) {
        const std::vector<int8_t> t2 = build_fir_table(f, r.mono2_pipe, true, e->mfma, msb, false);
        HIPCHK(e, e->d_fir_tables_m2.upload(t2.data(), t2.size()));
    }
    // the scratch: a line of 4096 stage-A integers per stream (the cascade: behind the P carried ones; two-pass 32-bit taps: one line per pass)
    if (e->cascade()) {
        const std::vector<int8_t> rt = build_resamp2_table(*e->fc.resamp);
        HIPCHK(e, e->d_resamp.upload(rt.data(), rt.size()));
        e->xs_hist = (uint32_t)e->fc.resamp->P;
    }
    if (e->mixed()) HIPCHK(e, e->d_mix.upload(e->mix.data(), e->mix.size() * sizeof(int32_t)));
    if (e->half) e->xs_hist = HALF_HIST;
    if (e->route.fine || e->cascade() || e->noise_shape || e->mixed() || e->half)
        HIPCHK(e, e->d_scratch.alloc(sizeof(int32_t) * ((size_t)e->xs_hist + 4096) * e->nstreams * (e->route.fine ? 2u : 1u)));
    if (e->noise_shape) {
        for (int i = 0; i < 2; ++i) HIPCHK(e, e->d_ns[i].alloc(sizeof(double) * 2 * e->nstreams));
        HIPCHK(e, e->d_ns_dump.alloc(1024));
    }
    for (int b = 0; b < 2; ++b) HIPCHK(e, e->d_hist[b].alloc((size_t)e->nstreams * e->route.keep));
    HIPCHK(e, e->d_peak.alloc(sizeof(double) * e->nstreams));
    e->launch.njobs = (size_t)e->nstreams * (e->route.fine ? 2u : e->mono2_ok() ? 3u : 1u);
    HIPCHK(e, e->d_jobs.alloc(sizeof(StreamJob) * e->launch.njobs));
    HIPCHK(e, e->h_jobs.alloc(sizeof(StreamJob) * e->launch.njobs * JOB_SLOTS));
    for (int i = 0; i < JOB_SLOTS; ++i) HIPCHK(e, hipEventCreateWithFlags(&e->job_ev[i], hipEventDisableTiming));
    build_launch_state(e);
    return reset_state(e);
}

namespace d2d { thread_local const char* d2d_last_launched_kernel = nullptr; }

extern "C" {

const char* d2d_create_error(void) { return g_create_error.c_str(); }

int d2d_create(const d2d_params* params, uint32_t n_files, d2d_engine** out) { return d2d_create_mix(params, nullptr, n_files, out); }

static int create_engine(const d2d_params* params, const d2d_mix* mix, const bool half, uint32_t n_files, d2d_engine** out);
int d2d_create_mix(const d2d_params* params, const d2d_mix* mix, uint32_t n_files, d2d_engine** out) { return create_engine(params, mix, false, n_files, out); }
int d2d_create_half(const d2d_params* params, uint32_t n_files, d2d_engine** out) { return create_engine(params, nullptr, true, n_files, out); }
uint32_t d2d_half_factor(const d2d_engine* e) { return e && e->half ? 2u : 0u; }

static int create_engine(const d2d_params* params, const d2d_mix* mix, const bool half, uint32_t n_files, d2d_engine** out) {
    if (out) *out = nullptr;
    if (!params || !out) { g_create_error = "null argument"; return D2D_ERR_PARAM; }
    if (mix && mix->struct_size != sizeof(d2d_mix)) { g_create_error = "d2d_mix.struct_size mismatch"; return D2D_ERR_PARAM; }
    constexpr size_t legacy_size = offsetof(d2d_params, channel_first);           // ABI 1: no channel subset
    constexpr size_t abi3_size = offsetof(d2d_params, tap_bits);                  // ABI 2, 3: no tap grid (ABI 4 and 5 have today's size: reserved0 became debug_flags)
    if (params->struct_size != sizeof(d2d_params) && params->struct_size != legacy_size && params->struct_size != abi3_size) {
        g_create_error = "d2d_params.struct_size mismatch"; return D2D_ERR_PARAM;
    }
    if (n_files < 1 || n_files > 65535) { g_create_error = "Invalid file count"; return D2D_ERR_PARAM; }
    std::unique_ptr<d2d_engine> e(new d2d_engine());
    memset(&e->p, 0, sizeof(e->p));
    memcpy(&e->p, params, params->struct_size);
    e->p.struct_size = sizeof(d2d_params);
    e->n_files = n_files;
    e->half = half;
    if (mix) {
        // (the bounds come first: nothing is read past what they admit; validate_mix repeats them with the other refusals, in d2d_create's order)
        const char* why = mix_check(e->p.channels, mix->out_channels, mix->coef);
        if (why) { g_create_error = why; return D2D_ERR_PARAM; }
        e->Co = mix->out_channels;
        e->mix.assign(mix->coef, mix->coef + (size_t)mix->out_channels * e->p.channels);
    }
    const int rc = init_engine(e.get());
    if (rc != D2D_OK) { g_create_error = e->err; return rc; }
    *out = e.release();
    return D2D_OK;
}

void d2d_destroy(d2d_engine* e) {
    if (!e) return;
    hipSetDevice(e->p.device);
    hipDeviceSynchronize();
    delete e;
}

int d2d_reset(d2d_engine* e) {
    if (!e) return D2D_ERR_PARAM;
    hipSetDevice(e->p.device);
    hipDeviceSynchronize();
    return reset_state(e);
}

const char* d2d_last_error(const d2d_engine* e) { return e ? e->err.c_str() : "null engine"; }

size_t d2d_frame_bytes(const d2d_engine* e) { return e ? (size_t)e->epi.sample_bytes * e->Co : 0; }

uint32_t d2d_input_channels(const d2d_engine* e) { return e ? e->Cin : 0u; }

int d2d_get_mix(const d2d_engine* e, uint32_t* out_channels, int32_t* coef, size_t capacity) {
    if (!e || !out_channels) return D2D_ERR_PARAM;
    *out_channels = e->mixed() ? e->Co : 0u;
    if (e->mixed() && coef) {
        if (capacity < e->mix.size()) return D2D_ERR_CAPACITY;
        std::copy(e->mix.begin(), e->mix.end(), coef);
    }
    return D2D_OK;
}

size_t d2d_next_frames(const d2d_engine* e, uint32_t file, size_t L) {
    if (!e || file >= e->n_files) return 0;
    const FileState& f = e->files[file];
    uint64_t nfir1 = (f.pos + L) / (uint64_t)e->Mb;
    if (e->half) return (size_t)(e->frames_at(nfir1, res_outputs_after(e, nfir1)) - e->frames_at(f.nfir, f.nres));
    return e->fc.resamp ? (size_t)(res_outputs_after(e, nfir1) - f.nres) : (size_t)(nfir1 - f.nfir);
}

// The scratch grows by doubling, to a multiple of 4 integers per line.  Unlike every other buffer it carries state across the reallocation:
// the xs_hist samples in front of each line move to the new stride before the old buffer goes (which `nb` owning the new one keeps leak-free).
static int grow_scratch(d2d_engine* e, size_t need_stride, hipStream_t s) {
    const size_t old = e->scratch_stride();
    if (need_stride <= old) return D2D_OK;
    const size_t ns = (std::max(need_stride, old * 2) + 3) & ~(size_t)3;
    Buf<int32_t> nb;
    HIPCHK(e, nb.alloc(sizeof(int32_t) * ns * e->nstreams * (e->route.fine ? 2u : 1u)));
    const size_t P = (size_t)e->xs_hist;
    if (P) HIPCHK(e, hipMemcpy2DAsync(nb, ns * sizeof(int32_t), e->d_scratch, old * sizeof(int32_t),
                                      P * sizeof(int32_t), e->nstreams, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipStreamSynchronize(s));
    e->d_scratch = std::move(nb);       // (the old buffer leaves with nb)
    return D2D_OK;
}

int d2d_seek(d2d_engine* e, uint32_t file, uint64_t pos) {
    if (!e) return D2D_ERR_PARAM;
    if (file >= e->n_files) return e->fail(D2D_ERR_PARAM, "file out of range");
    HIPCHK(e, hipSetDevice(e->p.device));
    HIPCHK(e, hipDeviceSynchronize());
    int rc = clear_file_state(e, file);
    if (!rc) rc = fills_done(e);
    if (rc) return rc;
    FileState& st = e->files[file];
    st.pos = pos;
    st.nfir = pos / (uint64_t)e->Mb;
    st.nres = res_outputs_after(e, st.nfir);
    st.ns_unknown = e->noise_shape && pos > 0;
    return D2D_OK;
}

int d2d_tell(const d2d_engine* e, uint32_t file, uint64_t* pos, uint64_t* next_frame) {
    if (!e || file >= e->n_files) return D2D_ERR_PARAM;
    const FileState& st = e->files[file];
    if (pos) *pos = st.pos;
    if (next_frame) *next_frame = e->frames_at(st.nfir, st.nres);
    return D2D_OK;
}

// The oldest byte the first frame after position p can depend on, as a distance back from p (include/dsd2dxd_amd.h: the guarantee).
//   single filter: output n = p / Mb ends at byte (n + 1) Mb > p - Mb + Mb, its window reaches Wb further back: Wb + Mb;
//   composed polyphase: the carried history is sized for exactly this (d2d_create: keep);
//   cascade: frame F(p) reads stage-A outputs no older than p / Mb - P - 1; the oldest of them ends no earlier than
//   p - Mb - P Mb and its window reaches Wb further back: Wb + (P + 1) Mb.
//   halved engine: frame F(p) reads the HALF_HIST sums in front of its newest one, each of which needs what the above says of an output:
//   HALF_HIST more steps of Mb bytes (single filter), or of Mp / (8 Lp) bytes, rounded up (composed polyphase: Lp outputs per Mp bits).
size_t d2d_preroll_bytes(const d2d_engine* e) {
    if (!e) return 0;
    if (e->half && e->poly) return e->route.keep + ((size_t)HALF_HIST * (size_t)e->poly->Mp + 8u * (size_t)e->poly->Lp - 1u) / (8u * (size_t)e->poly->Lp) + 1u;
    if (e->half) return (size_t)e->Wb + ((size_t)HALF_HIST + 1u) * (size_t)e->Mb;
    if (e->poly) return e->route.keep;
    if (e->cascade()) return (size_t)e->Wb + ((size_t)e->fc.resamp->P + 1) * (size_t)e->Mb;
    return (size_t)e->Wb + (size_t)e->Mb;
}

size_t d2d_slice_align_bytes(const d2d_engine* e) {
    if (!e) return 0;
    if (!e->noise_shape) return 1;
    if (!e->fc.resamp) return (size_t)e->Mb * 8192u;
    // F(k A) = k (A / Mb) L / Mdn: whole for A / Mb a multiple of Mdn (L and Mdn are coprime), a multiple of 8192 once L's own powers of two are counted
    const uint64_t L = (uint64_t)e->fc.resamp->L, Mdn = (uint64_t)e->fc.resamp->Mdn;
    uint64_t g = 8192; while (L % g) g >>= 1;
    return (size_t)((uint64_t)e->Mb * Mdn * (8192 / g));
}

}  // extern "C"

namespace {

// What the plan step of a call hands to the steps after it.
struct CallPlan {
    struct File { uint64_t nfir1, nres1, nframes; };     // FIR / stage-B outputs once the call is done, frames the call yields
    std::vector<File> files;
    uint32_t max_nx = 0, max_frames = 0, max_L = 0;      // the longest file's FIR outputs, frames and bytes per channel
    uint32_t max_sums = 0;                               // halved engine: the longest file's new sums (a prime has them too, and no frames)
    bool run_fir = false;
    bool mono2 = false;                                  // the call goes through the mono pair
};

}  // namespace

// Plan: every file's checks and counts; no HIP call.  A failing file leaves every frames_out as it was.
static int plan_call(d2d_engine* e, d2d_file_io* io, const bool prime, CallPlan& pl) {
    const size_t fb = d2d_frame_bytes(e);
    const uint32_t n_files = e->n_files;
    // a prime runs a FIR only where its outputs carry over: stage A of the cascade.  Every other engine's prime plans no outputs at all (max_nx,
    // max_frames = 0), which is what keeps the FIR passes, the mono pair and the combining pass out of it.
    pl.run_fir = !prime || e->cascade() || e->half;
    pl.files.resize(n_files);
    // MONO2: every file's call splits into two equal halves of whole outputs and whole 16-byte chunks, long enough to hold the second half's history
    pl.mono2 = e->mono2_ok();
    for (uint32_t f = 0; f < n_files; ++f) {
        const FileState& st = e->files[f];
        const size_t L = io[f].bytes_per_channel;
        if (L >= (1ull << 31)) return e->fail(D2D_ERR_PARAM, "bytes_per_channel must be below 2 GiB per call");
        if (L && (!io[f].dsd || ((uintptr_t)io[f].dsd & 15))) return e->fail(D2D_ERR_PARAM, "dsd device pointer must be non-null and 16-byte aligned");
        CallPlan::File& pf = pl.files[f];
        pf.nfir1 = (st.pos + L) / (uint64_t)e->Mb;
        pf.nres1 = res_outputs_after(e, pf.nfir1);
        const uint64_t nx = pl.run_fir ? pf.nfir1 - st.nfir : 0;
        const uint64_t sums = e->sums_at(pf.nfir1, pf.nres1) - e->sums_at(st.nfir, st.nres);
        const uint64_t frames = prime ? 0 : e->half ? e->frames_at(pf.nfir1, pf.nres1) - e->frames_at(st.nfir, st.nres) : e->fc.resamp ? pf.nres1 - st.nres : nx;
        pf.nframes = frames;
        if (frames * fb > io[f].pcm_capacity_bytes) return e->fail(D2D_ERR_CAPACITY, "pcm buffer too small");
        if (frames && (!io[f].pcm || ((uintptr_t)io[f].pcm & 15))) return e->fail(D2D_ERR_PARAM, "pcm device pointer must be non-null and 16-byte aligned");
        if (frames && st.ns_unknown && ((e->fc.resamp ? st.nres : st.nfir) & 8191u))
            return e->fail(D2D_ERR_STATE, "noise-shaped dither after d2d_seek / d2d_prime: frames can only start at an index that is a multiple of 8192 "
                                          "(cut the stream at multiples of d2d_slice_align_bytes)");
        pl.max_nx = std::max<uint32_t>(pl.max_nx, (uint32_t)nx);
        pl.max_frames = std::max<uint32_t>(pl.max_frames, (uint32_t)frames);
        if (e->half) pl.max_sums = std::max<uint32_t>(pl.max_sums, (uint32_t)sums);
        pl.max_L = std::max<uint32_t>(pl.max_L, (uint32_t)L);
        if (pl.mono2) {     // (a mono engine: file f is stream f, and the job's nout is the FIR's)
            const uint64_t half = L / 2, nout = pf.nfir1 - st.nfir;
            pl.mono2 = (L % 2 == 0) && (half % 16 == 0) && (half % (uint64_t)e->Mb == 0) && half >= e->route.keep && (nout % 2 == 0) &&
                       (uint64_t)(uint32_t)st.nfir + (uint32_t)nout <= 0xFFFFFFFFull;
        }
    }
    pl.mono2 = pl.mono2 && pl.max_nx > 0;
    for (uint32_t f = 0; f < n_files; ++f) io[f].frames_out = (size_t)pl.files[f].nframes;       // (written once every file has passed its checks)
    return D2D_OK;
}

// A batch started together asks every file for the same dither words: the word depends on the seed, the channel and the output index, not on
// the file.  Files from this count on at one index share a table of the call's words (d2d_dither_words_kernel) instead of hashing each their
// own inside the FIR kernel; below it the fill kernel and the reads cost more than the hashes (measured at 1 to 64 files of the bench's length:
// the table wins every round from 48 on, profiles/dither_table_check.md).
#ifndef D2D_DITHER_TABLE_MIN_FILES
#define D2D_DITHER_TABLE_MIN_FILES 48    // (-DD2D_DITHER_TABLE_MIN_FILES=1: the A/B build the threshold was measured with)
#endif
constexpr uint32_t kDitherTableMinFiles = D2D_DITHER_TABLE_MIN_FILES;
// words per channel: the call's longest file in whole wave-tiles (a partial tile's lanes read past its outputs and drop what they read)
static uint32_t dither_table_stride(const d2d_engine* e, const CallPlan& pl) {
    const uint32_t tile = std::max<uint32_t>(e->launch.fir.tile, 1u);
    return (((pl.max_nx + tile - 1u) / tile) * tile + 1023u) & ~1023u;
}

// Does this call's FIR launch read its dither words from the table?  Decided per call: the launch is a resident stereo frame flavour of the fp6
// kernel with a dither at unit gain (what compiles the reading form: d2d_mx.h, mx_dither_table), and the files that produce outputs, at least kDitherTableMinFiles,
// all start at the same index.  first_file: one of them, whose job rows hold the keys and the index.
static bool dither_table_serves(const d2d_engine* e, const CallPlan& pl, const bool prime, uint32_t* first_file) {
    const FirLaunch& l = e->launch.fir;
    if (prime || e->poly || e->mixed() || e->half || pl.mono2 || !pl.run_fir || pl.max_nx == 0 || (e->p.debug_flags & D2D_DBG_NO_DITHER_TABLE)) return false;
    if (l.family != FIR_MX || l.unit < 0 || e->C != 2 || l.m.f.coop || l.m.f.mono2) return false;
    const int MB = l.t[0], NT = l.t[1], KIND = l.t[3], SBY = l.t[4], NPR = l.t[5], ND = l.t[6];
    if (!mx_dither_table(MB, NT, KIND, SBY, NPR, ND)) return false;
    uint32_t active = 0;
    uint64_t n0 = 0;
    for (uint32_t f = 0; f < e->n_files; ++f) {
        const uint64_t nfir = e->files[f].nfir;
        if (pl.files[f].nfir1 == nfir) continue;
        if (active == 0) { n0 = nfir; *first_file = f; }
        else if (nfir != n0) return false;
        ++active;
    }
    return active >= kDitherTableMinFiles;
}

// Buffers: what the call's sizes ask of the scratch, the cascade's f64 line, the planar copy and the dither words.  Each waits on the call's stream.
static int reserve_call_buffers(d2d_engine* e, const CallPlan& pl, hipStream_t s, const bool prime) {
    uint32_t first_file = 0;
    if (dither_table_serves(e, pl, prime, &first_file))
        HIPCHK(e, e->d_dither.reserve(sizeof(uint32_t) * e->C * dither_table_stride(e, pl), wait_stream(s)));
    if (e->cascade() || e->noise_shape || e->route.fine || e->mixed() || e->half) {
        int rc = grow_scratch(e, (size_t)e->xs_hist + (e->half ? pl.max_sums : e->poly ? pl.max_frames : pl.max_nx), s);
        if (rc) return rc;
    }
    if (!prime && e->noise_shape && e->cascade()) {
        const size_t ns = ((size_t)pl.max_frames + 8 + 1023) & ~(size_t)1023;
        HIPCHK(e, e->d_ys.reserve(sizeof(double) * ns * e->nstreams, wait_stream(s)));
    }
    if (e->route.deinterleave) {
        const size_t need = (((size_t)pl.max_L * e->Cin) + 4095) & ~(size_t)4095;
        HIPCHK(e, e->d_planar.reserve(need * e->n_files, wait_stream(s)));
    }
    return D2D_OK;
}

// Jobs: the table in the next pinned slot (the mono pair's and the second pass's rows behind the streams'), its copy to the device and the
// event that frees the slot.
static int enqueue_jobs(d2d_engine* e, const d2d_file_io* io, const CallPlan& pl, hipStream_t s, const bool prime) {
    const size_t fb = d2d_frame_bytes(e);
    const uint32_t C = e->C, n_files = e->n_files;
    const int slot = e->job_slot;
    e->job_slot = (slot + 1) % JOB_SLOTS;
    if (e->job_ev_used[slot]) HIPCHK(e, hipEventSynchronize(e->job_ev[slot]));
    StreamJob* hj = e->h_jobs + (size_t)slot * e->launch.njobs;
    const int cur = e->hist_cur;
    const size_t scratch_stride = e->scratch_stride(), planar_stride = e->planar_stride();
    for (uint32_t f = 0; f < n_files; ++f) {
        const FileState& st = e->files[f];
        const CallPlan::File& pf = pl.files[f];
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t sidx = f * C + c;
            StreamJob& j = hj[sidx];
            j.in = e->route.deinterleave ? e->d_planar + (size_t)f * planar_stride : (const uint8_t*)io[f].dsd;
            j.in_raw = e->route.deinterleave ? (const uint8_t*)io[f].dsd : nullptr;
            j.hist = e->d_hist[cur] + (size_t)sidx * e->route.keep;
            j.hist_next = e->d_hist[cur ^ 1] + (size_t)sidx * e->route.keep;
            j.out = prime ? nullptr : io[f].pcm;
            j.xs = e->d_scratch ? e->d_scratch + (size_t)sidx * scratch_stride + e->xs_hist : nullptr;
            j.peak = e->d_peak + sidx;
            j.L = io[f].bytes_per_channel;
            j.e0 = (int64_t)((st.nfir + 1) * (uint64_t)e->Mb) - (int64_t)st.pos;
            j.n0 = st.nfir;
            j.nout = (uint32_t)(pf.nfir1 - st.nfir);
            if (e->poly) { j.e0 = (int64_t)st.pos; j.n0 = st.nres; j.nout = (uint32_t)(pf.nres1 - st.nres); }   // (PxArgs::jobs)
            j.ch = e->c0 + c;
            j.och = c;
            j.m0 = st.nres;
            j.nres = e->fc.resamp && !prime ? (uint32_t)(pf.nres1 - st.nres) : 0;
            const uint64_t i0 = e->frames_at(st.nfir, st.nres);      // index the dither counter runs on
            const uint64_t k = dither_key64(e->p.seed, e->c0 + c);
            j.rng_kstep = (uint32_t)k | 1u;
            j.rng_key = (uint32_t)(k >> 32) + (uint32_t)(i0 >> 32) * j.rng_kstep;
            j.rng_lo0 = (uint32_t)i0;
        }
    }
    if (pl.mono2)
        for (uint32_t f = 0; f < n_files; ++f) {
            StreamJob ja = hj[f];
            const uint64_t half = ja.L / 2;
            ja.L = half; ja.nout /= 2; ja.ch = 0; ja.och = 0;
            StreamJob jb = ja;
            jb.ch = 1;
            jb.hist = ja.in + half - e->route.keep;                           // the end of the first half
            jb.out = (uint8_t*)ja.out + (size_t)ja.nout * fb;
            jb.rng_key = ja.rng_key + ja.nout;                          // (the kernel hashes (first half's index + key): the second half's indices lie nout further on)
            hj[e->nstreams + 2 * f] = ja; hj[e->nstreams + 2 * f + 1] = jb;
        }
    if (e->route.fine)
        for (uint32_t i = 0; i < e->nstreams; ++i) { hj[e->nstreams + i] = hj[i]; hj[e->nstreams + i].xs = hj[i].xs + (size_t)e->nstreams * scratch_stride; }
    HIPCHK(e, hipMemcpyAsync(e->d_jobs, hj, sizeof(StreamJob) * e->launch.njobs, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipEventRecord(e->job_ev[slot], s));
    e->job_ev_used[slot] = true;
    return D2D_OK;
}

// one FIR pass over every file: `max_nout` outputs per stream at the most
static int launch_fir_pass(d2d_engine* e, const FirLaunch& p, uint32_t max_nout, hipStream_t s) {
    static FirLauncher* const launchers[] = {launch_fir_lut, launch_fir_mfma, launch_fir_mfma2, launch_fir_mfma3, launch_fir_mx, launch_fir_px, launch_poly_plain};   // by FirFamily
    HIPCHK(e, launchers[p.family](p, max_nout, e->n_files, s));
    return D2D_OK;
}

// Launch: every kernel of the call, in stream order, inside the two profiling brackets.
static int launch_call(d2d_engine* e, const CallPlan& pl, hipStream_t s, const bool prime) {
    const LaunchState& l = e->launch;
    const uint32_t n_files = e->n_files, max_nx = pl.max_nx, max_frames = pl.max_frames;
    const uint32_t px_nout = e->half ? pl.max_sums : max_frames;       // what the composed polyphase pass makes: frames, or a halved engine's sums
    EventPairs::Pair* ps = nullptr;
    if (e->profiling && (max_nx || (prime && pl.max_L))) HIPCHK(e, e->step.open(s, &ps));
    if (e->route.deinterleave) HIPCHK(e, launch_deinterleave(e->d_jobs, n_files, e->Cin, e->C, pl.max_L, s));
    // the call's dither words, once for all its files: inside the step bracket, in front of the FIR bracket, which stays the kernel alone
    uint32_t dt_file = 0;
    const bool dtab = dither_table_serves(e, pl, prime, &dt_file);
    const uint32_t dt_stride = dither_table_stride(e, pl);
    if (dtab) HIPCHK(e, launch_dither_words(e->d_jobs, dt_file * e->C, e->C, max_nx, e->d_dither, dt_stride, s));

    EventPairs::Pair* pe = nullptr;
    if (e->profiling && max_nx) HIPCHK(e, e->prof.open(s, &pe));
    {   // (the composed polyphase pass makes the frames themselves; the mono pair converts the two halves of a call side by side)
        int rc;
        if (dtab) {
            FirLaunch f = l.fir;                  // the plan's launch with this call's table
            f.m.f.dither_words = e->d_dither; f.m.f.dither_stride = dt_stride;
            rc = launch_fir_pass(e, f, max_nx, s);
            if (!rc) ++e->dither_table_calls;
        } else
            rc = e->poly ? launch_fir_pass(e, l.fir, px_nout, s) : pl.mono2 ? launch_fir_pass(e, l.fir_m2, max_nx / 2, s) : launch_fir_pass(e, l.fir, max_nx, s);
        if (rc) return rc;
    }
    if ((e->poly ? px_nout : max_nx) && d2d_last_launched_kernel) e->launched = d2d_last_launched_kernel;
    if (e->route.fine && max_nx) {
        // second pass: the residual taps, into the second half of the scratch
        int rc = launch_fir_pass(e, l.fir_lo, max_nx, s);
        if (rc) return rc;
    }
    if (pe) HIPCHK(e, hipEventRecord(pe->second, s));
    if (e->route.fine && max_nx) {
        // the matrix-core kernels write 2 sum(q b) - 2^S, which is sum(q s) only for a table that sums to 2^S: the residual table sums to 0
        const int64_t lo_bias = e->route.kernel == D2D_KERNEL_LUT ? 0 : ((int64_t)1 << e->S);
        HIPCHK(e, launch_fine_combine(e->d_jobs, e->nstreams, max_nx, (size_t)e->nstreams * e->scratch_stride(), lo_bias, e->S + 8, e->epi, s));
    }
    if (e->cascade()) {
        if (!prime) {
            Rs2Args r = l.rs;
            if (e->noise_shape) { r.ys = e->d_ys; r.ys_stride = (uint32_t)e->ys_stride(); }
            HIPCHK(e, launch_resample2(r, *e->fc.resamp, max_frames, n_files, s));
        }
        HIPCHK(e, launch_xhist(e->d_jobs, e->nstreams, (uint32_t)e->fc.resamp->P, s));
    }
    if (e->noise_shape && !prime) {
        NoiseShapeArgs ns = l.ns;
        ns.state = e->d_ns[e->ns_cur]; ns.state_next = e->d_ns[e->ns_cur ^ 1];
        ns.max_nout = e->fc.resamp ? max_frames : max_nx;
        if (e->cascade()) { ns.ys = e->d_ys; ns.ys_stride = (uint32_t)e->ys_stride(); }
        // a stream whose call ends exactly on a segment boundary, or feeds nothing, writes no state: start the next buffer from the current one
        HIPCHK(e, hipMemcpyAsync(e->d_ns[e->ns_cur ^ 1], e->d_ns[e->ns_cur], sizeof(double) * 2 * e->nstreams, hipMemcpyDeviceToDevice, s));
        HIPCHK(e, launch_noise_shape(ns, s));
        e->ns_cur ^= 1;
    }
    // the mix pass: where the noise-shaping pass runs, and like it not on a prime
    if (e->mixed() && !prime)
        HIPCHK(e, launch_mix(e->d_jobs, e->d_mix, e->C, n_files, e->poly ? max_frames : max_nx, e->poly ? e->poly->S : e->S, e->epi, s));
    // the half pass: where the mix pass runs, not on a prime; the sums it carries move to the front of their lines on every call that made some
    if (e->half && pl.max_sums) {
        if (!prime) HIPCHK(e, launch_half(e->d_jobs, e->C, n_files, pl.max_sums, e->poly ? e->poly->S : e->S, e->epi, s));
        HIPCHK(e, launch_half_hist(e->d_jobs, e->nstreams, s));
    }
    HIPCHK(e, launch_history(e->d_jobs, e->nstreams, e->Cin, e->route.B, e->route.keep, s));
    if (ps) HIPCHK(e, hipEventRecord(ps->second, s));
    return D2D_OK;
}

// Commit: the call is enqueued; the files stand where it leaves them.
static void commit_call(d2d_engine* e, const d2d_file_io* io, const CallPlan& pl, hipStream_t s, const bool prime) {
    e->hist_cur ^= 1;
    for (uint32_t f = 0; f < e->n_files; ++f) {
        FileState& st = e->files[f];
        if (e->noise_shape) {
            // frames began on a segment boundary: the shaper's state is the uninterrupted conversion's from here on; a prime leaves it unknown
            if (prime) { if (io[f].bytes_per_channel) st.ns_unknown = true; }
            else if (io[f].frames_out) st.ns_unknown = false;
        }
        st.pos += io[f].bytes_per_channel;
        st.nfir = pl.files[f].nfir1;
        st.nres = pl.files[f].nres1;
    }
    e->last_stream = s;
}

// One call of every file: what d2d_translate_batch_device and d2d_prime_batch_device share.
// prime: the bytes are consumed and everything that carries over to the next call is updated (the planar copy the history is read from,
// stage A of the cascade with its carried outputs, the bit history), but no frames are produced and the peaks stay.
static int batch_call(d2d_engine* e, d2d_file_io* io, uint32_t n_files, hipStream_t s, const bool prime) {
    if (!io || n_files != e->n_files) return e->fail(D2D_ERR_PARAM, "file count does not match the engine");
    HIPCHK(e, hipSetDevice(e->p.device));
    CallPlan pl;
    int rc = plan_call(e, io, prime, pl);
    if (!rc) rc = reserve_call_buffers(e, pl, s, prime);
    if (!rc) rc = enqueue_jobs(e, io, pl, s, prime);
    if (!rc) rc = launch_call(e, pl, s, prime);
    if (!rc) commit_call(e, io, pl, s, prime);
    return rc;
}

extern "C" {

int d2d_translate_batch_device(d2d_engine* e, d2d_file_io* io, uint32_t n_files, void* hip_stream) {
    if (!e) return D2D_ERR_PARAM;
    return batch_call(e, io, n_files, (hipStream_t)hip_stream, false);
}

int d2d_prime_batch_device(d2d_engine* e, d2d_file_io* io, uint32_t n_files, void* hip_stream) {
    if (!e) return D2D_ERR_PARAM;
    return batch_call(e, io, n_files, (hipStream_t)hip_stream, true);
}

// Host memory the GPU can address itself (hipHostMalloc, hipHostRegister; device memory passes too): the kernels then read the DSD
// and write the frames over the link with no staging copy at all -- one pass in which upload, conversion and download overlap by
// construction.  Measured on the bench batch (tools/zero_copy_probe.py): 52.9 ms per step = 89.6 GB/s over the link (reads alone
// 54.7 GB/s, writes alone 44.4), against 61.7 ms through the sliced three-stream pipeline below.  D2D_HOST_STAGED=1 keeps the pipeline.
static bool device_view(const void* p, void** dev) {
    if (!p) return false;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if ((at.type == hipMemoryTypeHost || at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) && at.devicePointer &&
        ((uintptr_t)at.devicePointer & 15) == 0) {               // (the batch entry point wants 16-byte aligned buffers)
        *dev = at.devicePointer;
        return true;
    }
    return false;
}
static bool host_staged_forced(const d2d_engine* e) { return (e->p.debug_flags & D2D_DBG_HOST_STAGED) != 0; }

// the single-file staging (d_in, d_out) holds `need` bytes: doubling, in whole 4 KiB pages, once own_stream has let go of the old memory
static int reserve_staging(d2d_engine* e, Buf<uint8_t>& b, size_t need) {
    need = std::max<size_t>(need, 16);
    if (need > b.bytes) need = (std::max(need, b.bytes * 2) + 4095) & ~(size_t)4095;
    HIPCHK(e, b.reserve(need, wait_stream(e->own_stream)));
    return D2D_OK;
}

// the caller's input where the GPU cannot read it in place: a copy in d_in, enqueued on own_stream
static int stage_input(d2d_engine* e, const void* dsd, size_t in_bytes, const void** dev) {
    int rc = reserve_staging(e, e->d_in, in_bytes);
    if (rc) return rc;
    if (in_bytes) HIPCHK(e, hipMemcpyAsync(e->d_in, dsd, in_bytes, hipMemcpyHostToDevice, e->own_stream));
    *dev = e->d_in;
    return D2D_OK;
}

// the most output a call of n bytes per channel can yield: the engine never emits more than ceil(bytes*8/M)+1 frames per call
static size_t slice_out_bytes(const d2d_engine* e, size_t n) {
    const double ratio = e->fc.resamp ? (double)e->fc.resamp->L / (double)e->fc.resamp->Mdn / (double)e->M : 1.0 / (double)e->M;
    return ((size_t)((double)n * 8.0 * ratio) + 4) * d2d_frame_bytes(e);
}

int d2d_translate(d2d_engine* e, const uint8_t* dsd, size_t L, void* pcm, size_t cap, size_t* frames_out) {
    if (!e) return D2D_ERR_PARAM;
    if (frames_out) *frames_out = 0;
    if (e->n_files != 1) return e->fail(D2D_ERR_STATE, "d2d_translate needs a single-file engine");
    if (L && !dsd) return e->fail(D2D_ERR_PARAM, "null dsd pointer");
    HIPCHK(e, hipSetDevice(e->p.device));
    const size_t frames = d2d_next_frames(e, 0, L);
    const size_t out_bytes = frames * d2d_frame_bytes(e);
    if (out_bytes > cap) return e->fail(D2D_ERR_CAPACITY, "pcm buffer too small");
    if (out_bytes && !pcm) return e->fail(D2D_ERR_PARAM, "null pcm pointer");
    const size_t in_bytes = L * e->Cin;
    hipStream_t s = e->own_stream;
    void *vin = nullptr, *vout = nullptr;
    const bool direct = in_bytes && out_bytes && !host_staged_forced(e) && device_view(dsd, &vin) && device_view(pcm, &vout);
    d2d_file_io io{};
    io.dsd = vin; io.bytes_per_channel = L; io.pcm = vout; io.pcm_capacity_bytes = cap;
    if (!direct) {
        int rc = reserve_staging(e, e->d_out, out_bytes);
        if (!rc) rc = stage_input(e, dsd, in_bytes, &io.dsd);
        if (rc) return rc;
        io.pcm = e->d_out; io.pcm_capacity_bytes = e->d_out.bytes;
    }
    int rc = d2d_translate_batch_device(e, &io, 1, s);
    if (rc) return rc;
    if (!direct && out_bytes) HIPCHK(e, hipMemcpyAsync(pcm, e->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (frames_out) *frames_out = io.frames_out;
    return D2D_OK;
}

int d2d_prime(d2d_engine* e, const uint8_t* dsd, size_t L) {
    if (!e) return D2D_ERR_PARAM;
    if (e->n_files != 1) return e->fail(D2D_ERR_STATE, "d2d_prime needs a single-file engine");
    if (L && !dsd) return e->fail(D2D_ERR_PARAM, "null dsd pointer");
    if (L >= (1ull << 31)) return e->fail(D2D_ERR_PARAM, "bytes_per_channel must be below 2 GiB per call");
    if (!L) return D2D_OK;
    HIPCHK(e, hipSetDevice(e->p.device));
    hipStream_t s = e->own_stream;
    d2d_file_io io{};
    io.bytes_per_channel = L;
    void* vin = nullptr;
    if (!host_staged_forced(e) && device_view(dsd, &vin)) {
        io.dsd = vin;
    } else {
        int rc = stage_input(e, dsd, L * e->Cin, &io.dsd);
        if (rc) return rc;
    }
    int rc = batch_call(e, &io, 1, s, true);
    if (rc) { hipStreamSynchronize(s); return rc; }
    HIPCHK(e, hipStreamSynchronize(s));
    return D2D_OK;
}

int d2d_translate_batch_host(d2d_engine* e, d2d_file_io* io, uint32_t n_files, size_t slice) {
    if (!e) return D2D_ERR_PARAM;
    if (!io || n_files != e->n_files) return e->fail(D2D_ERR_PARAM, "file count does not match the engine");
    HIPCHK(e, hipSetDevice(e->p.device));
    const uint32_t C = e->Cin;                       // the uploads move whole input frames
    const size_t fb = d2d_frame_bytes(e);
    if (slice == 0) slice = 4u << 20;
    // whole planar blocks per slice, for ANY block size (-s takes any value, src/main.rs:75-78): every slice then
    // starts on a block-group boundary, which is what the kernels' addressing of a call assumes.  (No rounding to 16
    // bytes: the staging buffers are 256-byte aligned per file whatever the slice length.)
    if (e->route.B > 1) slice = std::max<size_t>(e->route.B, slice / e->route.B * e->route.B);
    size_t max_L = 0;
    // every file's whole call against its buffer before anything is staged: the pipeline below converts and downloads slice by slice, and a
    // buffer that only a later slice overflows would otherwise fail with earlier slices in the caller's memory and the files moved on
    for (uint32_t f = 0; f < n_files; ++f) {
        if (io[f].bytes_per_channel && !io[f].dsd) return e->fail(D2D_ERR_PARAM, "null dsd pointer");
        const size_t frames = d2d_next_frames(e, f, io[f].bytes_per_channel);
        if (frames * fb > io[f].pcm_capacity_bytes) return e->fail(D2D_ERR_CAPACITY, "pcm buffer too small");
        if (frames && !io[f].pcm) return e->fail(D2D_ERR_PARAM, "null pcm pointer");
    }
    for (uint32_t f = 0; f < n_files; ++f) {
        max_L = std::max(max_L, io[f].bytes_per_channel);
        io[f].frames_out = 0;
    }
    if (max_L == 0) return D2D_OK;
    if (!host_staged_forced(e)) {
        std::vector<d2d_file_io> vio(io, io + n_files);
        // one call for the whole batch: every file below the per-call limit, and the cascade's / noise shaper's / 32-bit taps' scratch for all
        // of it at once (4 B per stage-A sample, 8 more per output where the two combine; two int32 halves with 32-bit taps) within half of
        // the free device memory -- otherwise the sliced pipeline below, which needs one slice of scratch
        bool direct = max_L < (1ull << 31);
        if (direct && (e->cascade() || e->noise_shape || e->route.fine || e->mixed() || e->half)) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(e, hipMemGetInfo(&free_b, &total_b));
            const double per_stream = (double)max_L / (double)e->Mb * (e->cascade() && e->noise_shape ? 12.0 : e->route.fine ? 8.0 : 4.0);
            direct = per_stream * (double)e->nstreams < 0.5 * (double)free_b;
        }
        for (uint32_t f = 0; f < n_files && direct; ++f) {
            if (!io[f].bytes_per_channel) continue;
            void *vin = nullptr, *vout = nullptr;
            direct = device_view(io[f].dsd, &vin) && device_view(io[f].pcm, &vout);
            vio[f].dsd = vin; vio[f].pcm = vout;
        }
        if (direct) {
            hipStream_t s = e->own_stream;
            int rc = d2d_translate_batch_device(e, vio.data(), n_files, s);
            if (rc) { hipStreamSynchronize(s); return rc; }
            HIPCHK(e, hipStreamSynchronize(s));
            for (uint32_t f = 0; f < n_files; ++f) io[f].frames_out = vio[f].frames_out;
            return D2D_OK;
        }
    }
    // double-buffered staging, one 256-byte aligned slice per file; a buffer that has to grow waits for the whole device
    const size_t in_stride = (slice * C + 255) & ~(size_t)255;
    const size_t out_stride = (slice_out_bytes(e, slice) + 255) & ~(size_t)255;
    for (int b = 0; b < 2; ++b) {
        HIPCHK(e, e->hb_in[b].reserve(in_stride * n_files, wait_device()));
        HIPCHK(e, e->hb_out[b].reserve(out_stride * n_files, wait_device()));
    }
    if (!e->hb_stream[0]) {
        for (int i = 0; i < 3; ++i) HIPCHK(e, hipStreamCreateWithFlags(&e->hb_stream[i], hipStreamNonBlocking));
        for (int i = 0; i < 6; ++i) HIPCHK(e, hipEventCreateWithFlags(&e->hb_ev[i], hipEventDisableTiming));
    }
    hipStream_t s_in = e->hb_stream[0], s_c = e->hb_stream[1], s_out = e->hb_stream[2];
    hipEvent_t* in_done = e->hb_ev; hipEvent_t* comp_done = e->hb_ev + 2; hipEvent_t* out_done = e->hb_ev + 4;
    std::vector<size_t> done(n_files, 0);
    std::vector<d2d_file_io> dio(n_files);
    // (equal slices: ramping them up and down -- slice/8, /4, /2, full ... -- to shorten the first upload and the last download was
    // measured and is slower, 64.2 against 61.7 ms per step: the step is bound by the per-copy cost of 2 x 64 transfers per slice,
    // not by fill and drain; the link alone moves the batch both ways in 47 ms, tools/link_probe.py)
    const size_t nslices = (max_L + slice - 1) / slice;
    for (size_t k = 0; k < nslices; ++k) {
        const int b = (int)(k & 1);
        const size_t slice_k = slice;
        // upload: the staging buffer is free once the conversion of slice k-2 has read it
        if (k >= 2) HIPCHK(e, hipStreamWaitEvent(s_in, comp_done[b], 0));
        for (uint32_t f = 0; f < n_files; ++f) {
            const size_t L = std::min(slice_k, io[f].bytes_per_channel - done[f]);
            dio[f].dsd = e->hb_in[b] + in_stride * f;
            dio[f].bytes_per_channel = L;
            dio[f].pcm = e->hb_out[b] + out_stride * f;
            dio[f].pcm_capacity_bytes = out_stride;
            if (L) HIPCHK(e, hipMemcpyAsync(e->hb_in[b] + in_stride * f, (const uint8_t*)io[f].dsd + done[f] * C, L * C, hipMemcpyHostToDevice, s_in));
            done[f] += L;
        }
        HIPCHK(e, hipEventRecord(in_done[b], s_in));
        // conversion: after its upload, and after the download of slice k-2 has drained the output buffer
        HIPCHK(e, hipStreamWaitEvent(s_c, in_done[b], 0));
        if (k >= 2) HIPCHK(e, hipStreamWaitEvent(s_c, out_done[b], 0));
        int rc = d2d_translate_batch_device(e, dio.data(), n_files, s_c);
        if (rc) { hipDeviceSynchronize(); return rc; }
        HIPCHK(e, hipEventRecord(comp_done[b], s_c));
        // download
        HIPCHK(e, hipStreamWaitEvent(s_out, comp_done[b], 0));
        for (uint32_t f = 0; f < n_files; ++f) {
            const size_t bytes = dio[f].frames_out * fb;
            if (!bytes) continue;
            if ((io[f].frames_out + dio[f].frames_out) * fb > io[f].pcm_capacity_bytes || !io[f].pcm) {
                hipDeviceSynchronize();
                return e->fail(D2D_ERR_CAPACITY, "pcm buffer too small");
            }
            HIPCHK(e, hipMemcpyAsync((uint8_t*)io[f].pcm + io[f].frames_out * fb, e->hb_out[b] + out_stride * f, bytes, hipMemcpyDeviceToHost, s_out));
            io[f].frames_out += dio[f].frames_out;
        }
        HIPCHK(e, hipEventRecord(out_done[b], s_out));
    }
    HIPCHK(e, hipStreamSynchronize(s_out));
    HIPCHK(e, hipStreamSynchronize(s_c));
    e->last_stream = s_c;
    return D2D_OK;
}

int d2d_peak(d2d_engine* e, uint32_t file, uint32_t channel, double* peak_out) {
    if (!e || !peak_out) return D2D_ERR_PARAM;
    if (file >= e->n_files || channel >= e->Co) return e->fail(D2D_ERR_PARAM, "file/channel out of range");
    HIPCHK(e, hipSetDevice(e->p.device));
    HIPCHK(e, hipStreamSynchronize(e->last_stream));
    HIPCHK(e, hipMemcpy(peak_out, e->d_peak + (size_t)file * e->C + channel, sizeof(double), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_peak_dbfs(d2d_engine* e, uint32_t file, float* dbfs_out) {
    if (!e || !dbfs_out) return D2D_ERR_PARAM;
    double m = 0.0;
    for (uint32_t c = 0; c < e->Co; ++c) {
        double v = 0.0;
        int rc = d2d_peak(e, file, c, &v);
        if (rc) return rc;
        m = std::max(m, v);
    }
    *dbfs_out = (float)(20.0 * log10(m));   // may be -inf/NaN-free; the CLI skips NaN (dsd_levels main.rs:188)
    return D2D_OK;
}

int d2d_convert_stream(d2d_engine* e, d2d_read_fn read, void* ru, d2d_write_fn write, void* wu,
                       const volatile int* cancel, d2d_progress_fn progress, void* pu,
                       uint64_t total, size_t chunk) {
    if (!e) return D2D_ERR_PARAM;
    if (!read) return e->fail(D2D_ERR_PARAM, "null read callback");
    if (e->n_files != 1) return e->fail(D2D_ERR_STATE, "d2d_convert_stream needs a single-file engine");
    HIPCHK(e, hipSetDevice(e->p.device));
    if (chunk == 0) chunk = 1u << 22;
    if (e->route.B > 1) chunk = std::max<size_t>(e->route.B, chunk / e->route.B * e->route.B);   // whole planar blocks per read
    // Pinned staging, two deep: while the GPU uploads, converts and downloads chunk k, the host reads
    // chunk k+1 and writes chunk k-1 (the callbacks are the file and sink I/O).
    const size_t fb = d2d_frame_bytes(e);
    const size_t in_cap = chunk * e->Cin, out_cap = slice_out_bytes(e, chunk);
    struct Pinned {
        Buf<uint8_t, true> in[2], out[2];
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Pinned() { for (int b = 0; b < 2; ++b) if (ev[b]) hipEventDestroy(ev[b]); }
    } pin;
    for (int b = 0; b < 2; ++b) {
        HIPCHK(e, pin.in[b].alloc(std::max<size_t>(in_cap, 16)));
        HIPCHK(e, pin.out[b].alloc(std::max<size_t>(out_cap, 16)));
        HIPCHK(e, hipEventCreateWithFlags(&pin.ev[b], hipEventDisableTiming));
    }
    // the kernels read and write the pinned buffers themselves when the GPU can address them (they are hipHostMalloc'ed: it can)
    void* vin[2] = {nullptr, nullptr}; void* vout[2] = {nullptr, nullptr};
    const bool direct = !host_staged_forced(e) && device_view(pin.in[0], &vin[0]) && device_view(pin.in[1], &vin[1]) &&
                        device_view(pin.out[0], &vout[0]) && device_view(pin.out[1], &vout[1]);
    int rc = D2D_OK;
    if (!direct) {
        rc = reserve_staging(e, e->d_in, in_cap);
        if (!rc) rc = reserve_staging(e, e->d_out, out_cap);
        if (rc) return rc;
    }
    hipStream_t s = e->own_stream;
    size_t pend_bytes[2] = {0, 0};
    uint64_t pend_in[2] = {0, 0};
    bool pending[2] = {false, false};
    uint64_t done = 0;
    auto retire = [&](int b) -> int {                // wait for chunk in buffer b, hand it to the sink
        if (!pending[b]) return D2D_OK;
        HIPCHK(e, hipEventSynchronize(pin.ev[b]));
        pending[b] = false;
        if (write && pend_bytes[b]) {
            if (write(wu, pin.out[b], pend_bytes[b]) != 0) return e->fail(D2D_ERR_IO, "write callback failed");
        }
        done += pend_in[b];
        if (progress && total) {
            float pct = (float)(100.0 * (double)done / (double)total);
            if (pct >= 100.0f) pct = 99.99f;   // exactly 100 is reserved for the end (src/main.rs:417-418)
            progress(pu, pct);
        }
        return D2D_OK;
    };
    auto drain = [&]() { hipStreamSynchronize(s); pending[0] = pending[1] = false; };
    for (int b = 0;; b ^= 1) {
        if (cancel && *cancel) { drain(); return e->fail(D2D_ERR_CANCELLED, "Conversion cancelled"); }
        rc = retire(b);                              // buffer b was used two chunks ago
        if (rc) { drain(); return rc; }
        long got = read(ru, pin.in[b], chunk);
        if (got < 0) { drain(); return e->fail(D2D_ERR_IO, "read callback failed"); }
        if (got == 0) { rc = retire(b ^ 1); if (rc) { drain(); return rc; } break; }
        const size_t L = (size_t)got;
        d2d_file_io io{};
        io.dsd = vin[b]; io.bytes_per_channel = L;
        io.pcm = direct ? vout[b] : e->d_out; io.pcm_capacity_bytes = direct ? pin.out[b].bytes : e->d_out.bytes;
        if (!direct) rc = stage_input(e, pin.in[b], L * e->Cin, &io.dsd);
        if (!rc) rc = d2d_translate_batch_device(e, &io, 1, s);
        if (rc) { drain(); return rc; }
        pend_bytes[b] = io.frames_out * fb;
        pend_in[b] = (uint64_t)got;
        if (!direct && pend_bytes[b]) HIPCHK(e, hipMemcpyAsync(pin.out[b], e->d_out, pend_bytes[b], hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipEventRecord(pin.ev[b], s));
        pending[b] = true;
        rc = retire(b ^ 1);                          // the previous chunk: its write overlaps this chunk's GPU work
        if (rc) { drain(); return rc; }
    }
    if (progress) progress(pu, 100.0f);
    return D2D_OK;
}

int d2d_profile_enable(d2d_engine* e, int on) {
    if (!e) return D2D_ERR_PARAM;
    e->profiling = on != 0;
    return D2D_OK;
}

int d2d_profile_read(d2d_engine* e, double* ms_total, uint64_t* launches) {
    if (!e) return D2D_ERR_PARAM;
    HIPCHK(e, hipSetDevice(e->p.device));
    const size_t n = e->prof.used;
    double tot = 0.0;
    HIPCHK(e, e->prof.elapsed_ms(&tot));
    if (ms_total) *ms_total = tot;
    if (launches) *launches = n;
    return D2D_OK;
}

int d2d_profile_read_all(d2d_engine* e, double* fir_ms_total, double* step_ms_total, uint64_t* launches) {
    if (!e) return D2D_ERR_PARAM;
    HIPCHK(e, hipSetDevice(e->p.device));
    double tot = 0.0;
    HIPCHK(e, e->step.elapsed_ms(&tot));
    if (step_ms_total) *step_ms_total = tot;
    return d2d_profile_read(e, fir_ms_total, launches);
}

size_t d2d_tables_bytes(const d2d_engine* e) {
    return e ? sizeof(TableBlobHeader) + ((e->d_fir_tables.bytes + 15) & ~(size_t)15) + e->d_resamp.bytes : 0;
}

static TableBlobHeader make_header(const d2d_engine* e) {
    TableBlobHeader h{};
    h.magic = 0x54443244u; h.abi = D2D_ABI_VERSION; h.kernel = e->route.kernel; h.endianness = e->p.endianness;
    h.ntaps = (uint32_t)e->N; h.M = (uint32_t)e->M; h.scale_bits = (uint32_t)e->S; h.filter_type = (uint32_t)e->fc.fir->type;
    h.table_variant = e->route.table_variant;
    if (e->route.taps32) h.scale_bits = (uint32_t)(e->S + 8);      // the seven-digit fragments of the 32-bit taps
    if (e->poly) { h.ntaps = (uint32_t)e->poly->NP; h.M = (uint32_t)e->poly->Mp; h.scale_bits = (uint32_t)e->poly->S; h.filter_type = (uint32_t)'P'; }
    h.fir_bytes = e->d_fir_tables.bytes; h.resamp_bytes = e->d_resamp.bytes;
    return h;
}

int d2d_tables_export_device(d2d_engine* e, void* dst, size_t cap, void* hip_stream) {
    if (!e || !dst) return D2D_ERR_PARAM;
    if (e->route.fine) return e->fail(D2D_ERR_STATE, "an engine with 32-bit taps holds two tap tables; the blob format carries one");
    if (cap < d2d_tables_bytes(e)) return e->fail(D2D_ERR_CAPACITY, "table blob buffer too small");
    HIPCHK(e, hipSetDevice(e->p.device));
    hipStream_t s = (hipStream_t)hip_stream;
    TableBlobHeader h = make_header(e);
    uint8_t* p = (uint8_t*)dst;
    HIPCHK(e, hipMemcpyAsync(p, &h, sizeof(h), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipStreamSynchronize(s));   // h is a stack object
    p += sizeof(h);
    HIPCHK(e, hipMemcpyAsync(p, e->d_fir_tables, e->d_fir_tables.bytes, hipMemcpyDeviceToDevice, s));
    p += (e->d_fir_tables.bytes + 15) & ~(size_t)15;
    if (e->d_resamp) HIPCHK(e, hipMemcpyAsync(p, e->d_resamp, e->d_resamp.bytes, hipMemcpyDeviceToDevice, s));
    return D2D_OK;
}

int d2d_tables_import_device(d2d_engine* e, const void* src, size_t bytes, void* hip_stream) {
    if (!e || !src) return D2D_ERR_PARAM;
    if (e->route.fine) return e->fail(D2D_ERR_STATE, "an engine with 32-bit taps holds two tap tables; the blob format carries one");
    if (bytes < d2d_tables_bytes(e)) return e->fail(D2D_ERR_PARAM, "table blob too small");
    HIPCHK(e, hipSetDevice(e->p.device));
    hipStream_t s = (hipStream_t)hip_stream;
    TableBlobHeader h{}, want = make_header(e);
    HIPCHK(e, hipMemcpyAsync(&h, src, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (memcmp(&h, &want, sizeof(h)) != 0) return e->fail(D2D_ERR_PARAM, "table blob does not match this engine's configuration");
    const uint8_t* p = (const uint8_t*)src + sizeof(h);
    HIPCHK(e, hipMemcpyAsync(e->d_fir_tables, p, e->d_fir_tables.bytes, hipMemcpyDeviceToDevice, s));
    p += (e->d_fir_tables.bytes + 15) & ~(size_t)15;
    if (e->d_resamp) HIPCHK(e, hipMemcpyAsync(e->d_resamp, p, e->d_resamp.bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return D2D_OK;
}

int d2d_get_info(const d2d_engine* e, d2d_info* out) {
    if (!e || !out) return D2D_ERR_PARAM;
    memset(out, 0, sizeof(*out));
    out->decimation = (uint32_t)e->M; out->ntaps = (uint32_t)e->N; out->scale_bits = (uint32_t)e->S;
    if (e->fc.resamp) { out->resamp_L = e->fc.resamp->L; out->resamp_M = e->fc.resamp->Mdn; out->resamp_P = e->fc.resamp->P; }
    if (e->poly) {      // one polyphase filter: Lp outputs per Mp bits, NP taps per phase
        out->decimation = 0; out->ntaps = (uint32_t)e->poly->NP; out->scale_bits = (uint32_t)e->poly->S;
        out->resamp_L = (uint32_t)e->poly->Lp; out->resamp_M = (uint32_t)e->poly->Mp; out->resamp_P = (uint32_t)e->poly->NP;
    }
    out->kernel = e->route.kernel; out->abi_version = D2D_ABI_VERSION;
    strncpy(out->filter_name, e->poly ? e->poly->name : e->fc.fir->name, sizeof(out->filter_name) - 1);
    return D2D_OK;
}

// diagnostic, not part of the public header: per-phase wave-cycle sums of the MFMA kernel (D2D_DBG=16)
void d2d_debug_stamps(unsigned long long* out8) { hipDeviceSynchronize(); mfma_debug_stamps(out8); }
void d2d_debug_stamps2(unsigned long long* out8) { hipDeviceSynchronize(); mfma2_debug_stamps(out8); }
void d2d_debug_stamps3(unsigned long long* out8) { hipDeviceSynchronize(); mfma3_debug_stamps(out8); if (out8[3] == 0) mx_debug_stamps(out8); }

uint64_t d2d_dither_table_calls(const d2d_engine* e) { return e ? e->dither_table_calls : 0; }

const char* d2d_kernel_name(const d2d_engine* e) {
    if (!e) return "";
    if (!e->launched.empty()) return e->launched.c_str();      // what the last call launched; before the first call: what the dispatch will choose
    if (e->kname.empty()) e->kname = route_kernel_name(e->route, e->fc, e->plan_epi);
    return e->kname.c_str();
}

}  // extern "C"
