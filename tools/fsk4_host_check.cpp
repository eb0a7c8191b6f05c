// The 4FSK modem's host restatement (habdec_amd/csrc/host/fsk4.hpp) run stand-alone, for AddressSanitizer and UBSan on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I habdec_amd/csrc -I include tools/fsk4_host_check.cpp -o /tmp/fsk4_host_check
//   /tmp/fsk4_host_check
//
// It generates frames of both presets with the encoder, sends them as 4FSK at 8, 32 and 45.3 samples per symbol with noise, NaN, Inf and values beyond
// +-8 around them, pushes them through the restatement in one piece and in pushes of 1, 63, 64, 65 and 4097 samples (a frame across the slot ring's
// wrap among them), with a reset in front, and checks the outcomes it knows: the payloads come back, every cut gives the same frames, candidates and
// counters, noise alone delivers nothing, a frame descriptor the decoder cannot take is refused.  Exit status 0: every check held and no sanitizer spoke.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host/fsk4.hpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static std::mt19937 rng(4321);

static std::vector<uint8_t> payload_of(const hd_fsk4_frame& f, int k)
{
    std::vector<uint8_t> p(f.payload_bytes);
    for (auto& b : p) b = (uint8_t)rng();
    p[0] = (uint8_t)k;
    const uint32_t crc = hd::fsk4_crc16(p.data(), p.size() - 2);
    p[p.size() - 2] = (uint8_t)crc; p[p.size() - 1] = (uint8_t)(crc >> 8);
    return p;
}

// frames of `f` at the samples `starts`, continuous-phase tones of amplitude 1 over noise of `sigma`, n samples, cf32 interleaved
static std::vector<float> signal(const hd_fsk4_frame& f, const std::vector<std::vector<uint8_t>>& payloads, const std::vector<double>& starts, double fsd,
                                 double baud, double f0, double spacing, double sigma, size_t n)
{
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<float> iq(2 * n);
    for (auto& v : iq) v = (float)(sigma * g(rng));
    const double spb = fsd / baud, two_pi = 6.283185307179586;
    for (size_t k = 0; k < payloads.size(); ++k) {
        uint8_t bytes[2 + 64];
        const size_t len = hd::fsk4_encode(f, payloads[k].data(), bytes);
        CHECK(len == 2u + hd::fsk4_body_bytes(f.payload_bytes));
        double phase = 0;
        for (size_t i = (size_t)starts[k]; i < n; ++i) {
            const double m = ((double)i - starts[k]) / spb;
            if (m < 0) continue;
            if (m >= 4.0 * len) break;
            const size_t sym = (size_t)m, bit = 2 * sym;
            const uint32_t v = ((bytes[bit / 8] >> (7 - bit % 8)) & 1u) << 1 | ((bytes[(bit + 1) / 8] >> (7 - (bit + 1) % 8)) & 1u);
            phase += two_pi * (f0 + spacing * v) / fsd;
            iq[2 * i] += (float)std::cos(phase); iq[2 * i + 1] += (float)std::sin(phase);
        }
    }
    return iq;
}

struct Result { std::vector<hd_fsk4_rx> rx; std::vector<hd_fsk4_candidate> cand; hd_fsk4_counters st; };

static Result run(const hd_fsk4_frame& f, const std::vector<float>& iq, double fsd, double baud, double f0, double spacing, std::vector<size_t> cuts,
                  bool behind_reset = false, uint32_t chase_bits = 4)
{
    hd_fsk4_params prm;
    hd::fsk4_params_default(&prm);
    prm.chase_bits = chase_bits;
    hd::Fsk4Stream s;
    s.set_params(prm);
    s.host_rings(4097);
    CHECK(hd::fsk4_tables(f, s.tab));
    CHECK(hd::fsk4_modem(s.s, fsd, baud, f0, spacing, prm.window_q8) == HD_OK);
    if (behind_reset) {
        s.push_samples(iq.data(), std::min<size_t>(iq.size() / 2, 3000));
        s.scan();
        s.waiting.clear();
        s.reset();
    }
    const size_t n = iq.size() / 2;
    for (size_t at = 0, k = 0; at < n; ++k) {
        const size_t m = std::min(cuts[k % cuts.size()], n - at);
        s.push_samples(iq.data() + 2 * at, m);
        s.scan();
        at += m;
    }
    Result r;
    r.rx.assign(s.waiting.begin(), s.waiting.end());
    r.cand.assign(s.log.begin(), s.log.end());
    s.stats(&r.st, s.s.n, s.s.g);
    return r;
}

static bool same(const Result& a, const Result& b)
{
    if (a.rx.size() != b.rx.size() || a.cand.size() != b.cand.size() || std::memcmp(&a.st, &b.st, sizeof a.st)) return false;
    for (size_t i = 0; i < a.rx.size(); ++i) if (std::memcmp(&a.rx[i], &b.rx[i], sizeof a.rx[i])) return false;
    for (size_t i = 0; i < a.cand.size(); ++i) if (std::memcmp(&a.cand[i], &b.cand[i], sizeof a.cand[i])) return false;
    return true;
}

static Result all_cuts(const hd_fsk4_frame& f, const std::vector<float>& iq, double fsd, double baud, double f0, double spacing)
{
    const Result one = run(f, iq, fsd, baud, f0, spacing, {4097});
    for (size_t cut : {1u, 63u, 64u, 65u}) CHECK(same(run(f, iq, fsd, baud, f0, spacing, {cut}), one));
    CHECK(same(run(f, iq, fsd, baud, f0, spacing, {1, 63, 64, 65, 4097}), one));
    CHECK(same(run(f, iq, fsd, baud, f0, spacing, {4097}, true), one));
    return one;
}

int main()
{
    hd_fsk4_frame v1, v2, bad;
    CHECK(hd::fsk4_preset(HD_FSK4_HORUS_V1, &v1) && hd::fsk4_preset(HD_FSK4_HORUS_V2, &v2) && !hd::fsk4_preset(3, &bad));
    CHECK(hd::fsk4_symbols(v1.payload_bytes) == 180 && hd::fsk4_symbols(v2.payload_bytes) == 260);
    {
        hd::Fsk4Tab t;
        for (uint32_t poly : {0xC76u, 0x475u, 0x1C75u}) { bad = v1; bad.golay_poly = poly; CHECK(!hd::fsk4_tables(bad, t)); }
        bad = v1; bad.interleave_mul = 336; CHECK(!hd::fsk4_tables(bad, t));
        bad = v1; bad.payload_bytes = 33; CHECK(!hd::fsk4_tables(bad, t));
        bad = v1; bad.golay_poly = 0xAE3; CHECK(hd::fsk4_tables(bad, t));
        hd::Fsk4State s;
        CHECK(hd::fsk4_modem(s, 32000, 32000 / 7.9, 0, 100, 256) == HD_ERR_UNSUPPORTED && hd::fsk4_modem(s, 32000, 4000, 4000, 4000, 256) == HD_ERR_INVALID);
    }
    const double fsd = 32000.0;
    struct Case { const hd_fsk4_frame* f; double baud, f0, spacing; } cases[] = {
        {&v1, 4000.0, -6000.0, 4000.0}, {&v2, 4000.0, 0.0, 4000.0}, {&v1, 1000.0, -1500.0, 1000.0}, {&v2, 32000.0 / 45.3, -15999.0, 9000.0}};
    for (const Case& c : cases) {
        const double spb = fsd / c.baud;
        const uint32_t nsym = hd::fsk4_symbols(c.f->payload_bytes);
        const std::vector<std::vector<uint8_t>> pl = {payload_of(*c.f, 1), payload_of(*c.f, 2)};
        // the second frame right behind the first; at 8 samples per symbol it lies across slot 8192, where the restatement's ring wraps
        const double first = spb == 8.0 ? 8192.0 - 1.5 * nsym * spb : 3.4 * spb;
        const size_t n = (size_t)(first + (2 * nsym + 6) * spb);
        std::vector<float> iq = signal(*c.f, pl, {first, first + nsym * spb}, fsd, c.baud, c.f0, c.spacing, 0.25, n);
        const float specials[] = {NAN, INFINITY, -INFINITY, 8.0f, -8.0f, 8.5f, -1e30f, 1e-45f};
        for (size_t i = 0; i < 24 && i < (size_t)first; ++i) iq[2 * i + (i & 1)] = specials[i % 8];
        const Result r = all_cuts(*c.f, iq, fsd, c.baud, c.f0, c.spacing);
        std::printf("%.1f samples per symbol, %u symbols: %zu frames, %zu candidates behind the gate of %llu, %llu slots\n", spb, nsym, r.rx.size(), r.cand.size(),
                    (unsigned long long)r.st.candidates, (unsigned long long)r.st.slots);
        CHECK(r.rx.size() == 2);
        for (size_t k = 0; k < r.rx.size() && k < 2; ++k)
            CHECK(r.rx[k].payload_bytes == c.f->payload_bytes && !std::memcmp(r.rx[k].payload, pl[k].data(), pl[k].size()) && r.rx[k].phase == (r.rx[k].slot & 7u));
        CHECK(r.st.gate_passes == r.cand.size() && r.st.frames == 2 && r.st.slots == hd::fsk4_slots_before(r.st.F, r.st.samples));
    }
    // noise alone: candidates behind the gate, every one refused by its CRC or by max_corrected
    {
        const std::vector<float> iq = signal(v1, {}, {}, fsd, 4000.0, -6000.0, 4000.0, 1.0, 40000);
        const Result r = all_cuts(v1, iq, fsd, 4000.0, -6000.0, 4000.0);
        std::printf("noise: %llu candidates, %llu behind the gate, %llu CRC failures, %llu refused, %llu frames\n", (unsigned long long)r.st.candidates,
                    (unsigned long long)r.st.gate_passes, (unsigned long long)r.st.crc_failures, (unsigned long long)r.st.refused, (unsigned long long)r.st.frames);
        CHECK(r.st.candidates == 40000 - 7 - 8 * 179 && r.st.gate_passes > 0 && r.rx.empty() && r.st.gate_passes == r.st.crc_failures + r.st.refused);
        CHECK(same(run(v1, iq, fsd, 4000.0, -6000.0, 4000.0, {4097}, false, 0), run(v1, iq, fsd, 4000.0, -6000.0, 4000.0, {65}, false, 0)));
        CHECK(same(run(v1, iq, fsd, 4000.0, -6000.0, 4000.0, {4097}, false, 6), run(v1, iq, fsd, 4000.0, -6000.0, 4000.0, {63}, false, 6)));
    }
    std::printf(failures ? "%d checks FAILED\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
