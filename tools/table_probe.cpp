// table_probe.cpp -- every operand table of dsd2dxd_amd/csrc/d2d_tables.cpp on the host (tests/test_tables_cpu.py, tests/golden/table_digests.json).
//   g++ -O2 -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o table_probe table_probe.cpp ../dsd2dxd_amd/csrc/d2d_tables.cpp
// One line per table: "<key> <bytes> <64-bit FNV-1a of the bytes>"; the predicates and sums as "<key> <value>"; "<key> n/a" where a builder is
// not defined for a filter (fp6 digits below M = 32, seven digits without half32 or where mx_wide_exact fails).  Keys:
//   <filter>[.residual]/<L|M>/<lut|one_group|two_group|pipelined|fp6|fp6_wide>     L / M: the stream's bit order; .residual: residual_def(filter)
//   <filter>[.residual]/<mx_exact|mx_wide_exact|sum_abs_q>
//   <poly>/<px|px_exact|max_phase_sum_abs>      <resampler>/<resamp2|nstep>
// (mfma_supported holds for every M of D2D_FILTERS, so the one-group table is printed for all of them.)
#include <stdio.h>

#include <string>
#include <vector>

#include "../dsd2dxd_amd/csrc/d2d_tables.h"

using namespace d2d;

template <class T>
static void table(const std::string& key, const std::vector<T>& t) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(t.data());
    for (size_t i = 0; i < t.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    printf("%s %zu %016llx\n", key.c_str(), t.size() * sizeof(T), (unsigned long long)h);
}
static void value(const std::string& key, unsigned long long v) { printf("%s %llu\n", key.c_str(), v); }
static void none(const std::string& key) { printf("%s n/a\n", key.c_str()); }

static void filter(const std::string& name, const d2d_filter_def& f) {
    const bool wide = f.half32 && f.M >= 32 && mx_wide_exact(f);
    for (int msb = 0; msb < 2; ++msb) {
        const std::string k = name + (msb ? "/M/" : "/L/");
        table(k + "lut", build_lut_tables(f, f.M / 8, msb));
        table(k + "one_group", build_mfma_tables(f, mfma_layout(f.M, f.ntaps), msb));
        table(k + "two_group", build_mfma2_tables(f, msb, true));
        table(k + "pipelined", build_mfma2_tables(f, msb, false));
        if (f.M >= 32) table(k + "fp6", build_mx_tables(f, msb, false)); else none(k + "fp6");
        if (wide) table(k + "fp6_wide", build_mx_tables(f, msb, true)); else none(k + "fp6_wide");
    }
    value(name + "/mx_exact", mx_exact(f));
    value(name + "/mx_wide_exact", mx_wide_exact(f));
    value(name + "/sum_abs_q", sum_abs_q(f));
}

int main() {
    for (const d2d_filter_def& f : D2D_FILTERS) {
        filter(f.name, f);
        if (!f.half32) continue;
        std::vector<int32_t> half;
        filter(std::string(f.name) + ".residual", residual_def(f, half));
    }
    for (const d2d_poly_def& p : D2D_POLYS) {
        const std::string k = std::string(p.name) + "/";
        table(k + "px", build_px_tables(p));
        value(k + "px_exact", px_exact(p));
        value(k + "max_phase_sum_abs", max_phase_sum_abs(p));
    }
    for (const d2d_resamp_def& r : D2D_RESAMPLERS) {
        const std::string k = std::string(r.name) + "/";
        table(k + "resamp2", build_resamp2_table(r));
        value(k + "nstep", resamp2_nstep(r));
    }
    return 0;
}
