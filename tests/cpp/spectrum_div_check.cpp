// tests/test_spectrum_div.py: hd::specwave::spec_div (kernels/spectrum_math.h) against the division it replaces, (float)((double)q / rate), bit for bit.
// Prints one line per rate: "rate <r> checked <n> mismatches <m> normal <k> slow <j>" (normal / slow: the strided inputs that are positive normal
// floats with a normal float quotient, and how many of them took the division), and the first mismatches, if any, on stderr.
#include <initializer_list>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "kernels/spectrum_math.h"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()      // splitmix64
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Tally { uint64_t checked = 0, mismatches = 0, normal = 0, slow = 0; };

static void check(Tally& t, const double rate, const double rinv, const float q, const bool count_slow)
{
    const volatile double quotient = (double)q / rate;      // (volatile: the reference is this division, whatever the optimiser thinks of it)
    const float want = (float)quotient;
    bool slow = false;
    const float got = hd::specwave::spec_div(q, rate, rinv, &slow);
    ++t.checked;
    if (bits_of(want) != bits_of(got)) {
        if (t.mismatches < 8) fprintf(stderr, "rate %.17g q %a (0x%08x): division 0x%08x, spec_div 0x%08x, slow %d\n", rate, (double)q, bits_of(q), bits_of(want), bits_of(got), (int)slow);
        ++t.mismatches;
    }
    if (count_slow && q >= 0x1p-126f && q < INFINITY && quotient >= 0x1p-126 && quotient < 0x1p128) {
        ++t.normal;
        if (slow) ++t.slow;
    }
}

static void around(Tally& t, const double rate, const double rinv, const float q)      // q and its two neighbours on each side
{
    float lo = q, hi = q;
    check(t, rate, rinv, q, false);
    for (int i = 0; i < 2; ++i) {
        lo = nextafterf(lo, -INFINITY); hi = nextafterf(hi, INFINITY);
        check(t, rate, rinv, lo, false); check(t, rate, rinv, hi, false);
    }
}

int main()
{
    const double rates[] = {32000.0, 156250.0, 39062.5, 512000.0, 8000.0};
    const uint32_t stride = 1021;                                    // odd, below 2^10: 4.2e6 patterns
    for (const double rate : rates) {
        const double rinv = 1.0 / rate;
        Tally t;
        // every float bit pattern at the stride, both signs, NaNs and infinities as they come
        for (uint64_t u = 0; u < (1ull << 32); u += stride) check(t, rate, rinv, float_of((uint32_t)u), true);
        // zeros, infinities, a NaN; the subnormal inputs' ends and the inputs whose quotient is at the ends of the subnormal floats
        const float special[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 0x1p-149f, 0x1p-126f, -0x1p-149f, -0x1p-126f, 3.4028234663852886e38f,
                                 (float)(0x1p-149 * rate), (float)(0x1p-150 * rate), (float)(0x1p-126 * rate), (float)(0x1p-127 * rate), (float)(0x1.fffffep127 * rate > 3.4e38 ? 3.4e38 : 0x1.fffffep127 * rate)};
        for (const float q : special) {
            check(t, rate, rinv, q, false);
            if (q == q && q - q == 0.0f) around(t, rate, rinv, q);
        }
        // every subnormal input of either sign with the normal floats next to them, and (rate > 1: consecutive inputs give every quotient there) a stretch of
        // consecutive inputs across the quotient 2^-126, the end of the subnormal results
        for (uint32_t u = 0; u < (1u << 23) + 16; ++u) { check(t, rate, rinv, float_of(u), false); check(t, rate, rinv, float_of(u | 0x80000000u), false); }
        {
            const uint32_t c = bits_of((float)(0x1p-126 * rate));
            for (uint32_t u = c - (1u << 15); u < c + (1u << 15); ++u) check(t, rate, rinv, float_of(u), false);
        }
        // the adversarial inputs of the guard: for random float results f, the floats nearest to (f + ulp/2) * rate -- quotients next to a rounding midpoint
        for (int i = 0; i < 1000000; ++i) {
            const uint64_t r = rng();
            const uint32_t e = 127 - 100 + (uint32_t)((r >> 32) % 200);               // 2^-100 .. 2^100: input and quotient are both normal floats
            const float f = float_of((e << 23) | ((uint32_t)r & 0x7FFFFFu));
            const double mid = (double)f + 0.5 * ((double)nextafterf(f, INFINITY) - (double)f);
            around(t, rate, rinv, (float)(mid * rate));
        }
        printf("rate %.17g checked %llu mismatches %llu normal %llu slow %llu\n", rate, (unsigned long long)t.checked, (unsigned long long)t.mismatches,
               (unsigned long long)t.normal, (unsigned long long)t.slow);
    }
    // The rates above have few significant bits, and a 24-bit input over such a rate cannot come closer to a midpoint than about one part in 2^32: the
    // guard is never needed there.  So, beyond them, rates made for it: for a random input q and a random midpoint, rate = q / midpoint rounded to double
    // and its two neighbours on each side put the quotient within a few units of the last place of that midpoint, on either side of it.
    {
        Tally t;
        uint64_t slow_taken = 0;
        for (int i = 0; i < 1000000; ++i) {
            const uint64_t r = rng(), r2 = rng();
            const float q = float_of(((127 - 40 + (uint32_t)((r >> 32) % 80)) << 23) | ((uint32_t)r & 0x7FFFFFu));
            const float f = float_of(((127 - 40 + (uint32_t)((r2 >> 32) % 80)) << 23) | ((uint32_t)r2 & 0x7FFFFFu));
            const double mid = (double)f + 0.5 * ((double)nextafterf(f, INFINITY) - (double)f);
            double lo = (double)q / mid, hi = lo;
            for (int k = 0; k < 3; ++k) {
                for (const double rate : {lo, hi}) {
                    bool slow = false;
                    (void)hd::specwave::spec_div(q, rate, 1.0 / rate, &slow);
                    slow_taken += slow;
                    check(t, rate, 1.0 / rate, q, false);
                }
                lo = nextafter(lo, 0.0); hi = nextafter(hi, INFINITY);
            }
        }
        printf("constructed checked %llu mismatches %llu slow %llu\n", (unsigned long long)t.checked, (unsigned long long)t.mismatches, (unsigned long long)slow_taken);
    }
    return 0;
}
