// Host program of tests/test_upsample_sorted_host.py: csrc/sample_cdf.h (invert_cdf_at and the lane test of k_upsample) compiled as plain C++.
// Each case builds a row of new depths the way k_upsample does - invert_cdf_at of an ascending u over one CDF - and prints
//     <case> n=<row length> truth=<sorted|unsorted> verdict=<sorted|unsorted>
// truth: a plain scan of the row written here (ascending, no NaN); verdict: lane_row_in_order on all 64 lanes, combined as the kernel's ballot does.
#include "sample_cdf.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

using nerfart::invert_cdf_at;
using nerfart::lane_row_in_order;

static std::vector<float> invert_row(const std::vector<float>& bins, const std::vector<float>& cdf, const std::vector<float>& u) {
    std::vector<float> out(u.size());
    for (size_t j = 0; j < u.size(); ++j) out[j] = invert_cdf_at(bins.data(), cdf.data(), (int)bins.size(), u[j]);
    return out;
}

static bool truth_sorted(const std::vector<float>& r) {
    for (float v : r) if (std::isnan(v)) return false;
    for (size_t j = 0; j + 1 < r.size(); ++j) if (r[j] > r[j + 1]) return false;
    return true;
}

static bool verdict_sorted(const std::vector<float>& r) {
    bool all = true;
    for (int lane = 0; lane < 64; ++lane) all = lane_row_in_order(r.data(), (int)r.size(), lane) && all;
    return all;
}

static int report(const char* name, const std::vector<float>& r) {
    const bool t = truth_sorted(r), v = verdict_sorted(r);
    std::printf("%s n=%zu truth=%s verdict=%s\n", name, r.size(), t ? "sorted" : "unsorted", v ? "sorted" : "unsorted");
    return 0;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

// A row of 512 ascending u in which sample `at` is u_hit and sample at + 1 is u_next; the rest is a linspace that stays clear of both.
static std::vector<float> u_row(int at, float u_hit, float u_next) {
    std::vector<float> u(512);
    for (int j = 0; j < 512; ++j) {
        if (j <= at) u[j] = u_hit * (float)(j + 1) / (float)(at + 1);
        else if (j > at + 1) u[j] = u_next + (0.999f - u_next) * (float)(j - at - 1) / (float)(511 - at - 1);
    }
    u[at] = u_hit; u[at + 1] = u_next;
    return u;
}

// The break all of these are built around: u equal to the CDF entry c2 gives t = 1 exactly and b0 + 1 * (b1 - b0), which for many (b0, b1) is one
// ulp ABOVE b1; the next sample falls just behind c2 and comes out as b1 when its own term t * (b2 - b1) is below half an ulp of b1.  `kind` chooses
// why that term is so small.  Searches (b0, b1) until the row really is out of order; returns false if no draw did.
static bool planted(const char* name, int kind, int at) {
    uint32_t seed = 12345u + 977u * (uint32_t)kind + (uint32_t)at;
    for (int draw = 0; draw < 4096; ++draw) {
        const float b0 = 0.5f + 3.0f * unit(seed), b1 = 4.0f + 1.5f * unit(seed);
        const float c1 = 0.3f, c2 = 0.6f;
        float b2, c3, u_next;
        if (kind == 0) {              // a run of (nearly) equal CDF values: the denominator 2e-6 is below 1e-5 and becomes 1
            b2 = b1 + 1e-3f; c3 = c2 + 2e-6f; u_next = c2 + 1e-6f;
        } else if (kind == 1) {       // a bin one ulp wide
            b2 = std::nextafter(b1, 10.f); c3 = 0.8f; u_next = 0.61f;
        } else {                      // nothing special about the bin: the next u is simply the next float behind the CDF entry
            b2 = b1 + 0.25f; c3 = 0.8f; u_next = std::nextafter(c2, 1.f);
        }
        const std::vector<float> bins = {0.f, b0, b1, b2, 6.f}, cdf = {0.f, c1, c2, c3, 1.f};
        const std::vector<float> row = invert_row(bins, cdf, u_row(at, c2, u_next));
        if (row[at] > row[at + 1]) { report(name, row); return true; }
    }
    std::printf("%s: no (b0, b1) draw broke the order\n", name);
    return false;
}

int main() {
    bool ok = true;
    // out of order by construction; the pair sits inside a lane's stride, at a wave boundary (lane 63 -> lane 0 of the next 64) and at the row's end
    const int ats[] = {5, 63, 127, 300, 510};
    char name[64];
    for (int at : ats) {
        std::snprintf(name, sizeof(name), "equal_run_at_%d", at);      ok = planted(name, 0, at) && ok;
        std::snprintf(name, sizeof(name), "one_ulp_bin_at_%d", at);    ok = planted(name, 1, at) && ok;
        std::snprintf(name, sizeof(name), "u_on_cdf_entry_at_%d", at); ok = planted(name, 2, at) && ok;
    }
    // NaN: one depth of the old row is NaN (one sample of the new row), and a whole row of NaN (identical bits everywhere)
    {
        std::vector<float> bins(1024), cdf(1024), u(512);
        for (int i = 0; i < 1024; ++i) { bins[i] = 6.f * (float)i / 1023.f; cdf[i] = (float)i / 1023.f; }
        for (int j = 0; j < 512; ++j) u[j] = (float)(j + 1) / 513.f;
        std::vector<float> b = bins;
        b[400] = std::numeric_limits<float>::quiet_NaN();
        report("nan_one_bin", invert_row(b, cdf, u));
        std::vector<float> row = invert_row(bins, cdf, u);
        row[511] = std::numeric_limits<float>::quiet_NaN();
        report("nan_last_element", row);
        row.assign(512, std::numeric_limits<float>::quiet_NaN());
        report("nan_everywhere", row);
        std::vector<float> z(512, 0.f);
        z[100] = -0.f;
        report("minus_zero_among_zeros", z);         // ascending as numbers: the verdict is the stricter one, a sort could move the -0
    }
    // in order: linspace u over smooth CDFs, the shapes the sampler's rounds have (1,024 / 1,536 / 512 old samples, 512 new ones)
    for (int n : {512, 1024, 1536}) {
        for (int shape = 0; shape < 3; ++shape) {
            std::vector<float> bins(n), cdf(n), u(512);
            double run = 0.0, total = 0.0;
            std::vector<double> w(n - 1);
            for (int k = 0; k < n - 1; ++k) {
                const double x = (k + 0.5) / (n - 1);
                w[k] = shape == 0 ? 1.0 : (shape == 1 ? 1e-5 + std::exp(-0.5 * (x - 0.4) * (x - 0.4) / (0.02 * 0.02)) : 0.05 + x * x);
                total += w[k];
            }
            cdf[0] = 0.f;
            for (int k = 0; k < n - 1; ++k) { run += w[k] / total; cdf[k + 1] = (float)run; }
            for (int i = 0; i < n; ++i) bins[i] = 6.f * (float)i / (float)(n - 1);
            for (int j = 0; j < 512; ++j) u[j] = (float)(j + 1) / 513.f;
            std::snprintf(name, sizeof(name), "smooth_n%d_shape%d", n, shape);
            report(name, invert_row(bins, cdf, u));
        }
    }
    return ok ? 0 : 1;
}
