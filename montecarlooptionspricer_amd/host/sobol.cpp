// Host side of the Sobol' generators (include/mcgpu.h: mcg_sobol_table, mcg_sobol_bridge, mcg_rqmc_combine): the direction
// numbers with their scramble, the bridge schedule, and the replicate error bar.  Plain C++, no HIP header: it builds and runs
// without the runtime (tests/cpp/sobol_host_main.cpp, under the sanitizers); the error channel is the library's mcg::fail, which
// that program supplies itself.  include/mcgpu.h states every rule that is restated here.
#include <cmath>
#include <vector>

#include "../../include/mcgpu.h"
#include "sobol_joe_kuo.hpp"

namespace mcg {
int fail(int status, const char* fmt, ...);

static_assert(SOBOL_TABLE_DIMS == MCG_SOBOL_MAX_DIMS, "tools/gen_sobol_table.py and include/mcgpu.h disagree");

// what the table, the bridge and the four generators reject of their mcg_sobol alike
int sobol_check(const mcg_sobol* s) {
    if (!s) return fail(MCG_ERR_INVALID, "sobol is NULL");
    if (s->scramble < MCG_SOBOL_PLAIN || s->scramble > MCG_SOBOL_LMS_SHIFT)
        return fail(MCG_ERR_INVALID, "sobol: scramble must be 0 (plain), 1 (shift) or 2 (matrix scramble + shift), got %d", s->scramble);
    if (s->bridge != 0 && s->bridge != 1) return fail(MCG_ERR_INVALID, "sobol: bridge must be 0 or 1 (got %d)", s->bridge);
    return MCG_OK;
}

// ... and of the shape of their matrix; n_steps < 1 and n_paths < 0 are left to the model's own checks
int sobol_check_shape(const mcg_sobol* s, int n_steps, uint64_t path_begin, int64_t n_paths) {
    const int rc = sobol_check(s);
    if (rc) return rc;
    if (n_steps > MCG_SOBOL_MAX_DIMS)
        return fail(MCG_ERR_INVALID, "sobol: n_steps must be <= %d, one dimension per step (got %d)", MCG_SOBOL_MAX_DIMS, n_steps);
    const uint64_t points = 1ull << 32;
    if (n_paths > 0 && (path_begin > points || (uint64_t)n_paths > points - path_begin))
        return fail(MCG_ERR_INVALID, "sobol: path_begin + n_paths must be <= 2^32 (got %llu + %lld)", (unsigned long long)path_begin,
                    (long long)n_paths);
    return MCG_OK;
}

namespace {

inline uint64_t splitmix_next(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t splitmix_hash(uint64_t x) { return splitmix_next(x); }
inline uint32_t word(uint64_t& s) { return (uint32_t)(splitmix_next(s) >> 32); }

// V[d][0 .. 31] of Joe and Kuo's recurrence, leading digit in bit 31
void direction_numbers(int d, uint32_t* v) {
    const unsigned poly = SOBOL_POLY[d];
    int s = 0;
    while ((poly >> (s + 1)) != 0) ++s;  // degree
    uint32_t m[32];
    if (s == 0) {
        for (int j = 0; j < 32; ++j) m[j] = 1u;
    } else {
        for (int j = 0; j < s; ++j) m[j] = SOBOL_MINIT[d][j];
        for (int j = s; j < 32; ++j) {
            uint32_t x = m[j - s] ^ (m[j - s] << s);
            for (int k = 1; k < s; ++k)
                if ((poly >> (s - k)) & 1u) x ^= m[j - k] << k;
            m[j] = x;
        }
    }
    for (int j = 0; j < 32; ++j) v[j] = m[j] << (31 - j);
}

inline uint32_t parity(uint32_t x) {
    x ^= x >> 16;
    x ^= x >> 8;
    x ^= x >> 4;
    x ^= x >> 2;
    x ^= x >> 1;
    return x & 1u;
}

}  // namespace
}  // namespace mcg

using namespace mcg;

extern "C" int mcg_sobol_table(const mcg_sobol* sobol, int n_dims, uint32_t* v_out, uint32_t* shift_out) {
    int rc = sobol_check(sobol);
    if (rc) return rc;
    if (!v_out || !shift_out) return fail(MCG_ERR_INVALID, "sobol: v_out/shift_out is NULL");
    if (n_dims < 1 || n_dims > MCG_SOBOL_MAX_DIMS)
        return fail(MCG_ERR_INVALID, "sobol: n_dims must be in [1, %d] (got %d)", MCG_SOBOL_MAX_DIMS, n_dims);
    uint64_t state = splitmix_hash(splitmix_hash(sobol->seed) ^ (uint64_t)sobol->replicate);
    for (int d = 0; d < n_dims; ++d) {
        uint32_t* v = v_out + (size_t)d * 32;
        direction_numbers(d, v);
        if (sobol->scramble == MCG_SOBOL_PLAIN) {
            shift_out[d] = 0u;
            continue;
        }
        shift_out[d] = word(state);
        uint32_t mask[32];
        for (int j = 0; j < 32; ++j) mask[j] = ((word(state) >> (31 - j)) | 1u) << (31 - j);
        if (sobol->scramble != MCG_SOBOL_LMS_SHIFT) continue;
        for (int b = 0; b < 32; ++b) {
            uint32_t x = 0u;
            for (int j = 0; j < 32; ++j) x |= parity(mask[j] & v[b]) << (31 - j);
            v[b] = x;
        }
    }
    return MCG_OK;
}

extern "C" int mcg_sobol_bridge(int n_steps, int bridge, mcg_bridge_node* out) {
    if (!out) return fail(MCG_ERR_INVALID, "sobol bridge: out is NULL");
    if (n_steps < 1 || n_steps > MCG_SOBOL_MAX_DIMS)
        return fail(MCG_ERR_INVALID, "sobol bridge: n_steps must be in [1, %d] (got %d)", MCG_SOBOL_MAX_DIMS, n_steps);
    if (bridge != 0 && bridge != 1) return fail(MCG_ERR_INVALID, "sobol: bridge must be 0 or 1 (got %d)", bridge);
    if (!bridge) {
        for (int d = 0; d < n_steps; ++d) out[d] = mcg_bridge_node{d + 1, d, d, 1.0, 0.0, 1.0};
        return MCG_OK;
    }
    out[0] = mcg_bridge_node{n_steps, 0, 0, 0.0, 0.0, std::sqrt((double)n_steps)};
    // breadth first: the intervals of a level in the order of the level above, `out` itself is the queue of those that
    // have a node (entries 1 ..); an interval without one (r - l < 2) has no children
    int head = 1, tail = 1;
    auto push = [&](int l, int r) {
        if (r - l < 2) return;
        const int m = (l + r) / 2;
        const double w = (double)(r - l);
        out[tail++] = mcg_bridge_node{m, l, r, (double)(r - m) / w, (double)(m - l) / w, std::sqrt((double)(m - l) * (double)(r - m) / w)};
    };
    push(0, n_steps);
    while (head < tail) {
        const mcg_bridge_node e = out[head++];
        push(e.l, e.t);
        push(e.t, e.r);
    }
    return MCG_OK;
}

extern "C" int mcg_rqmc_combine(const double* estimates, int n, double* mean, double* std_err) {
    if (!estimates || !mean || !std_err) return fail(MCG_ERR_INVALID, "rqmc combine: a NULL argument");
    if (n < 2) return fail(MCG_ERR_INVALID, "rqmc combine: at least two replicates make an error bar (got %d)", n);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += estimates[i];
    const double m = sum / (double)n;
    double ss = 0.0;
    for (int i = 0; i < n; ++i) ss += (estimates[i] - m) * (estimates[i] - m);
    *mean = m;
    *std_err = std::sqrt(ss / (double)(n - 1) / (double)n);
    return MCG_OK;
}
