// The two 4096-entry {cos, sin} tables of fm::sincos_two_level (csrc/fastmath.hpp): the 24-bit Box-Muller angle
// f = ((wb >> 8) + 1/2) 2^-24 split 12 + 12,
//   coarse[i] = {cos, sin}(2 pi i / 4096)              i = wb >> 20
//   fine[j]   = {cos, sin}(2 pi (j + 1/2) / 2^24)      j = (wb >> 8) & 4095
// so that cos/sin(2 pi f) is one complex product.  Built once per process in long double (64-bit significand) and rounded
// to binary64: each entry is within 1/2 ulp + the long-double evaluation error of the true value.  The coarse angles are
// reduced to the first octant in INTEGERS before anything is rounded (k <= 512 of 4096: the argument of sinl / cosl is at
// most pi/4, where both keep their relative accuracy; the exact entries 0, +-1 and the equal pair at odd multiples of
// pi/4 come out exactly so), the fine ones lie below 2 pi 2^-12 and need no reduction.
#include <cmath>
#include <mutex>

#include "../csrc/mcg_internal.hpp"

namespace mcg {

namespace {

constexpr long double TWO_PI_L = 6.283185307179586476925286766559005768L;

void octant_entry(int i, double& c_out, double& s_out) {
    const int oct = i >> 9, k = i & 511;       // angle = oct * pi/4 + 2 pi k / 4096
    const bool flip = (oct & 1) != 0;          // odd octants: measure the angle back from the octant's upper end
    const int kk = flip ? 512 - k : k;         // 0 .. 512
    const long double t = TWO_PI_L * (long double)kk / 4096.0L;
    long double c = cosl(t), s = sinl(t);      // of an angle in [0, pi/4]
    if (kk == 0) {
        c = 1.0L;
        s = 0.0L;
    }
    if (flip) std::swap(c, s);                 // the angle inside its quadrant is pi/2 - t
    // quadrant q = oct >> 1: rotate by q * pi/2
    switch (oct >> 1) {
        case 0: break;
        case 1: { const long double x = c; c = -s; s = x; break; }
        case 2: c = -c; s = -s; break;
        default: { const long double x = c; c = s; s = -x; break; }
    }
    c_out = (double)c + 0.0;                   // (+ 0.0: no negative zero in the table)
    s_out = (double)s + 0.0;
}

struct Sincos2Host {
    double coarse[2 * SINCOS2_ENTRIES], fine[2 * SINCOS2_ENTRIES];
};

}  // namespace

const double* host_sincos2_tables() {
    static Sincos2Host* tabs = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        Sincos2Host* t = new Sincos2Host;
        for (int i = 0; i < SINCOS2_ENTRIES; ++i) {
            octant_entry(i, t->coarse[2 * i], t->coarse[2 * i + 1]);
            const long double a = TWO_PI_L * ((long double)i + 0.5L) / 16777216.0L;
            t->fine[2 * i] = (double)cosl(a);
            t->fine[2 * i + 1] = (double)sinl(a);
        }
        tabs = t;
    });
    return tabs->coarse;
}

}  // namespace mcg

extern "C" int mcg_debug_sincos2_tables(double* coarse, double* fine) {
    using namespace mcg;
    if (!coarse || !fine) return fail(MCG_ERR_INVALID, "coarse or fine is NULL");
    const double* t = host_sincos2_tables();
    std::copy(t, t + 2 * SINCOS2_ENTRIES, coarse);
    std::copy(t + 2 * SINCOS2_ENTRIES, t + 4 * SINCOS2_ENTRIES, fine);
    return MCG_OK;
}
