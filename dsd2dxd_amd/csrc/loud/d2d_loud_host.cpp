// d2d_loud_host.cpp -- the host half of the loudness calls (include/dsd2dxd_amd.h, "Loudness where the PCM is"): the K-weighting
// coefficients, d2d_loud_measure_host, the CPU twin of the GPU call on loud_meter.h, and the integration behind both twins (gates,
// ReplayGain; d2d_loud_finish_album: the same gates over the blocks of several meters); d2d_true_peak_measure_host, the CPU twin of the
// true-peak call on true_peak.h, and the meter's true-peak side.  No HIP:
// tools and tests build this file with g++ alone.
#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "d2d_loud_internal.h"

using namespace d2dloud;

namespace {

// a0 and the two feedback coefficients of a second-order section with this K and Q
void feedback(double K, double Q, double& a0, double& a1, double& a2) {
    a0 = 1.0 + K / Q + K * K;
    a1 = 2.0 * (K * K - 1.0) / a0;
    a2 = (1.0 - K / Q + K * K) / a0;
}

Coef coefficients(uint32_t rate) {
    const double pi = 3.14159265358979323846;
    Coef k;
    {   // the shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / (double)rate), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        double a0;
        feedback(K, Q, a0, k.sa1, k.sa2);
        k.sb0 = (Vh + Vb * K / Q + K * K) / a0;
        k.sb1 = 2.0 * (K * K - Vh) / a0;
        k.sb2 = (Vh - Vb * K / Q + K * K) / a0;
    }
    {   // the high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / (double)rate);
        double a0;
        feedback(K, Q, a0, k.ha1, k.ha2);
        k.hb0 = 1.0; k.hb1 = -2.0; k.hb2 = 1.0;
    }
    return k;
}

inline uint32_t raw_le(const uint8_t* p, uint32_t sb) {
    uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    if (sb > 2) v |= (uint32_t)p[2] << 16;
    if (sb > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

}  // namespace


struct d2d_loud {
    uint32_t channels = 0, rate = 0;
    double weights[8] = {0};
    double last[3][8] = {{0}};                                     // the energies of the three sub-blocks before the next one, oldest first
    uint64_t subblocks = 0;
    bool ended = false;                                            // a partial row was added: the stream is over
    double peak = 0.0;
    std::vector<double> power;                                     // sum_c G_c z_c of every 400 ms block, in order
    // true peak (d2d_loud_set_true_peak): off, nothing below is touched
    bool tp_on = false;
    bool started = false;                                          // an add of either kind was accepted: the switch is fixed
    uint64_t tp_subblocks = 0;
    bool tp_ended = false;
    double tp_peak = 0.0;                                          // the largest double added
};

namespace d2dloud {
Coef host_coefficients(uint32_t rate) { return coefficients(rate); }
uint32_t meter_rate(const d2d_loud* h) { return h->rate; }
uint32_t meter_channels(const d2d_loud* h) { return h->channels; }
bool meter_true_peak(const d2d_loud* h) { return h->tp_on; }
}  // namespace d2dloud

extern "C" {

int d2d_loud_coefficients(uint32_t rate, double out[10]) {
    if (!rate_ok(rate)) return fail(D2D_ERR_PARAM, "loudness is measured at rates that are a multiple of 10 in 8000 .. 1411200");
    if (!out) return fail(D2D_ERR_PARAM, "null coefficients");
    const Coef k = coefficients(rate);
    static_assert(sizeof(Coef) == 10 * sizeof(double), "ten doubles");
    memcpy(out, &k, sizeof(k));
    return D2D_OK;
}

int d2d_loud_measure_host(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_loud_io* io) {
    const int rc = check_call(channels, bit_depth, rate);
    if (rc != D2D_OK) return rc;
    if (!io) return fail(D2D_ERR_PARAM, "no file");
    if (io->frames == 0) return D2D_OK;
    Plan p;
    const int prc = plan_file(*io, channels, rate, 1, p);
    if (prc != D2D_OK) return prc;
    const Coef k = coefficients(rate);
    const uint32_t sb = sample_bytes(bit_depth);
    const size_t fb = (size_t)channels * sb;
    const uint8_t* pcm = (const uint8_t*)io->pcm;
    const uint64_t end = io->first_frame + io->frames;
    for (uint64_t r = 0; r < p.rows(); ++r) {
        const uint64_t j = io->first_subblock + r;
        const uint64_t from = start_subblock(j) * p.S, at = j * p.S, to = at + p.S < end ? at + p.S : end;
        for (uint32_t c = 0; c < channels; ++c) {
            Unit u;
            const uint8_t* q = pcm + (size_t)(from - io->first_frame) * fb + (size_t)c * sb;
            for (uint64_t f = from; f < at; ++f, q += fb) preroll(u, k, sample(raw_le(q, sb), bit_depth));
            for (uint64_t f = at; f < to; ++f, q += fb) measure(u, k, sample(raw_le(q, sb), bit_depth));
            d2d_loud_cell cell{u.energy, u.peak};
            memcpy((uint8_t*)io->cells + ((size_t)r * channels + c) * sizeof(cell), &cell, sizeof(cell));      // (cells need no alignment here)
        }
    }
    write_counts(*io, p, channels);
    return D2D_OK;
}

int d2d_loud_create(uint32_t channels, uint32_t rate, const double* weights, d2d_loud** out) {
    if (!out) return fail(D2D_ERR_PARAM, "null meter pointer");
    if (channels == 0 || channels > 8) return fail(D2D_ERR_PARAM, "loudness is measured on 1 to 8 channels (Invalid channel count)");
    if (!rate_ok(rate)) return fail(D2D_ERR_PARAM, "loudness is measured at rates that are a multiple of 10 in 8000 .. 1411200");
    d2d_loud* h = new (std::nothrow) d2d_loud();
    if (!h) return fail(D2D_ERR_STATE, "out of memory");
    h->channels = channels; h->rate = rate;
    static const double six[6] = {1.0, 1.0, 1.0, 0.0, 1.41, 1.41};           // L R C LFE Ls Rs
    for (uint32_t c = 0; c < channels; ++c) h->weights[c] = weights ? weights[c] : (channels == 6 ? six[c] : 1.0);
    *out = h;
    return D2D_OK;
}

int d2d_loud_add(d2d_loud* h, const d2d_loud_cell* cells, size_t whole_subblocks, int has_partial) {
    if (!h) return fail(D2D_ERR_PARAM, "null meter");
    if (!cells && (whole_subblocks || has_partial)) return fail(D2D_ERR_PARAM, "null cells");
    if (h->ended && (whole_subblocks || has_partial)) return fail(D2D_ERR_STATE, "cells behind the partial sub-block that ended the stream");
    h->started = true;
    const uint32_t ch = h->channels;
    const double four_s = 4.0 * (double)(h->rate / 10);
    for (size_t r = 0; r < whole_subblocks; ++r) {
        d2d_loud_cell row[8];
        memcpy(row, (const uint8_t*)cells + r * ch * sizeof(d2d_loud_cell), ch * sizeof(d2d_loud_cell));
        for (uint32_t c = 0; c < ch; ++c)
            if (row[c].peak > h->peak) h->peak = row[c].peak;
        if (h->subblocks >= 3) {                                   // the block that ends with this sub-block
            double w = 0.0;
            for (uint32_t c = 0; c < ch; ++c) {
                const double e = ((h->last[0][c] + h->last[1][c]) + h->last[2][c]) + row[c].energy;
                const double z = e / four_s;
                w = w + h->weights[c] * z;
            }
            h->power.push_back(w);
        }
        for (uint32_t c = 0; c < ch; ++c) { h->last[0][c] = h->last[1][c]; h->last[1][c] = h->last[2][c]; h->last[2][c] = row[c].energy; }
        ++h->subblocks;
    }
    if (has_partial) {                                             // its peak only
        d2d_loud_cell row[8];
        memcpy(row, (const uint8_t*)cells + whole_subblocks * ch * sizeof(d2d_loud_cell), ch * sizeof(d2d_loud_cell));
        for (uint32_t c = 0; c < ch; ++c)
            if (row[c].peak > h->peak) h->peak = row[c].peak;
        h->ended = true;
    }
    return D2D_OK;
}

// the two gates over the blocks of `n` meters, in meter order then block order: what d2d_loud_finish (n = 1) and d2d_loud_finish_album share
static d2d_loud_result integrate(const d2d_loud* const* meters, uint32_t n_meters) {
    d2d_loud_result r{};
    for (uint32_t i = 0; i < n_meters; ++i) {
        if (meters[i]->peak > r.peak) r.peak = meters[i]->peak;
        r.blocks_total += meters[i]->power.size();
    }
    auto lufs = [](double w) { return -0.691 + 10.0 * log10(w); };
    // the absolute gate
    double sum = 0.0; uint64_t n = 0;
    for (uint32_t i = 0; i < n_meters; ++i)
        for (double w : meters[i]->power)
            if (w > 0.0 && lufs(w) > -70.0) { sum = sum + w; ++n; }
    if (n) {
        const double relative = lufs(sum / (double)n) - 10.0;
        double kept = 0.0; uint64_t m = 0;
        for (uint32_t i = 0; i < n_meters; ++i)
            for (double w : meters[i]->power)
                if (w > 0.0 && lufs(w) > -70.0 && lufs(w) > relative) { kept = kept + w; ++m; }
        r.valid = 1;                                               // (the loudest block lies above the mean less 10 LU: m > 0)
        r.lufs = lufs(kept / (double)m);
        r.gain_db = -18.0 - r.lufs;
        r.blocks_gated = r.blocks_total - m;
    } else r.blocks_gated = r.blocks_total;
    return r;
}

int d2d_loud_finish(const d2d_loud* h, d2d_loud_result* result) {
    if (!h || !result) return fail(D2D_ERR_PARAM, "null meter or result");
    *result = integrate(&h, 1);
    return D2D_OK;
}

// the meters of an album: at least one, none null, all of one channel count, rate and weights
static int check_album(const d2d_loud* const* meters, uint32_t n) {
    if (!meters || n == 0) return fail(D2D_ERR_PARAM, "an album has at least one meter");
    for (uint32_t i = 0; i < n; ++i) {
        if (!meters[i]) return fail(D2D_ERR_PARAM, "null meter");
        if (meters[i]->channels != meters[0]->channels || meters[i]->rate != meters[0]->rate ||
            memcmp(meters[i]->weights, meters[0]->weights, sizeof(meters[0]->weights)))
            return fail(D2D_ERR_PARAM, "meter " + std::to_string(i) + " differs from meter 0 in channels, rate or weights");
    }
    return D2D_OK;
}

int d2d_loud_finish_album(const d2d_loud* const* meters, uint32_t n, d2d_loud_result* result) {
    if (!result) return fail(D2D_ERR_PARAM, "null meter or result");
    const int rc = check_album(meters, n);
    if (rc != D2D_OK) return rc;
    *result = integrate(meters, n);
    return D2D_OK;
}

int d2d_loud_true_peak_album(const d2d_loud* const* meters, uint32_t n, double* out) {
    if (!out) return fail(D2D_ERR_PARAM, "null meter or result");
    const int rc = check_album(meters, n);
    if (rc != D2D_OK) return rc;
    double largest = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        double v = 0.0;
        const int prc = d2d_loud_true_peak(meters[i], &v);
        if (prc != D2D_OK) return prc;
        if (v > largest) largest = v;
    }
    *out = largest;
    return D2D_OK;
}

void d2d_loud_destroy(d2d_loud* h) { delete h; }

int d2d_true_peak_measure_host(uint32_t channels, uint32_t bit_depth, uint32_t rate, d2d_tpeak_io* io) {
    const int rc = check_call(channels, bit_depth, rate);
    if (rc != D2D_OK) return rc;
    if (!io) return fail(D2D_ERR_PARAM, "no file");
    if (io->frames == 0) return D2D_OK;
    Plan p;
    const int prc = plan_tpeak_file(*io, channels, rate, 1, 1, p);
    if (prc != D2D_OK) return prc;
    const uint32_t sb = sample_bytes(bit_depth);
    const size_t fb = (size_t)channels * sb;
    const uint8_t* pcm = (const uint8_t*)io->pcm;
    const uint64_t end = io->first_frame + io->frames;
    std::vector<double> x(d2dtp::HISTORY + (size_t)p.S);              // a sub-block of one channel behind its history, in time order
    for (uint64_t r = 0; r < p.rows(); ++r) {
        const uint64_t j = io->first_subblock + r;
        const uint64_t at = j * p.S, to = at + p.S < end ? at + p.S : end;
        for (uint32_t c = 0; c < channels; ++c) {
            for (uint32_t k = 0; k < d2dtp::HISTORY; ++k) {               // frames at - 11 .. at - 1: zeros before the stream
                const uint64_t back = d2dtp::HISTORY - k;
                x[k] = at >= back ? sample(raw_le(pcm + (size_t)(at - back - io->first_frame) * fb + (size_t)c * sb, sb), bit_depth) : 0.0;
            }
            const uint8_t* q = pcm + (size_t)(at - io->first_frame) * fb + (size_t)c * sb;
            for (uint64_t f = at; f < to; ++f, q += fb) x[d2dtp::HISTORY + (size_t)(f - at)] = sample(raw_le(q, sb), bit_depth);
            double m = 0.0;
            for (size_t i = 0; i < (size_t)(to - at); ++i) {
                const double y = d2dtp::frame_peak(&x[d2dtp::HISTORY + i]);
                if (y > m) m = y;
            }
            const double peak = m * d2dtp::SCALE;
            memcpy((uint8_t*)io->peaks + ((size_t)r * channels + c) * sizeof(double), &peak, sizeof(double));      // (peaks need no alignment here)
        }
    }
    write_tpeak_counts(*io, p, channels);
    return D2D_OK;
}

int d2d_loud_set_true_peak(d2d_loud* h, int on) {
    if (!h) return fail(D2D_ERR_PARAM, "null meter");
    if (h->started) return fail(D2D_ERR_PARAM, "true peak is switched before the meter's first add");
    h->tp_on = on != 0;
    return D2D_OK;
}

int d2d_loud_add_true_peaks(d2d_loud* h, const double* peaks, size_t whole_subblocks, int has_partial) {
    if (!h) return fail(D2D_ERR_PARAM, "null meter");
    if (!h->tp_on) return fail(D2D_ERR_PARAM, "the meter's true peak is not switched on (d2d_loud_set_true_peak)");
    if (!peaks && (whole_subblocks || has_partial)) return fail(D2D_ERR_PARAM, "null peaks");
    if (h->tp_ended && (whole_subblocks || has_partial)) return fail(D2D_ERR_STATE, "peaks behind the partial sub-block that ended the stream");
    h->started = true;
    const size_t n = (whole_subblocks + (has_partial ? 1 : 0)) * h->channels;
    for (size_t i = 0; i < n; ++i) {
        double v;
        memcpy(&v, (const uint8_t*)peaks + i * sizeof(double), sizeof(double));
        if (v > h->tp_peak) h->tp_peak = v;
    }
    h->tp_subblocks += whole_subblocks;
    if (has_partial) h->tp_ended = true;
    return D2D_OK;
}

int d2d_loud_true_peak(const d2d_loud* h, double* out) {
    if (!h || !out) return fail(D2D_ERR_PARAM, "null meter or result");
    if (!h->tp_on || (h->tp_subblocks == 0 && !h->tp_ended)) return fail(D2D_ERR_PARAM, "no true-peak rows were added");
    if (h->tp_subblocks != h->subblocks || h->tp_ended != h->ended)
        return fail(D2D_ERR_PARAM, "the true-peak rows added are not the rows of cells added");
    *out = h->tp_peak > h->peak ? h->tp_peak : h->peak;
    return D2D_OK;
}

}  // extern "C"
