// The 4FSK tone tracker's and the retune's host restatement (habdec_amd/csrc/host/fsk4_track.hpp, host/fsk4.hpp) run stand-alone, for AddressSanitizer and
// UBSan on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I habdec_amd/csrc -I include tools/fsk4_track_host_check.cpp -o /tmp/fsk4_track_host_check
//   /tmp/fsk4_track_host_check
//
// It runs the detector on built spectra -- four lobes, lobes whose windows touch the band's edges and the spectrum's first and last bins, all zeros, a
// NaN, a negative bin, the narrowest and the widest plans -- and the tracker with a modem attached on twelve frames whose tones drift, whole and in pushes
// of 1, 63, 64, 65 and 4097 samples, and checks the outcomes it knows: every cut gives the same records, sums, retunes and frames, the frames come back,
// refusals refuse.  Exit status 0: every check held and no sanitizer spoke.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host/fsk4_track.hpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static std::mt19937 rng(9876);
static const double FSD = 32000.0, BAUD = 1000.0, SP = 2700.0, BIN = FSD / 4096.0;

static std::vector<double> lobes(const std::vector<double>& centres, double width, double base)
{
    std::vector<double> a(4096, base);
    for (double c : centres)
        for (int k = 0; k < 4096; ++k) a[k] += std::max(0.0, 1.0 - std::fabs(k - c) / width);
    return a;
}

static void detector()
{
    hd::Fsk4CombPlan pl;
    hd_fsk4_comb_record r;
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 4 * BAUD, -12000, 12000, pl) == HD_OK);
    hd::fsk4_comb_detect(lobes({1500.3, 1845.9, 2191.5, 2537.1}, 100, 0.01).data(), pl, 192, true, &r);
    CHECK(r.valid == 1 && std::abs(r.f0_q8 - (int32_t)(1500.3 * 256)) < 64 && std::abs(r.spacing_q8 - (int32_t)(345.6 * 256)) < 32);
    hd::fsk4_comb_detect(lobes({1500.3, 1845.9, 2537.1}, 100, 0.01).data(), pl, 192, true, &r);
    CHECK(r.valid == 0);
    std::vector<double> z(4096, 0.0);
    hd::fsk4_comb_detect(z.data(), pl, 0, true, &r);
    CHECK(r.valid == 0 && r.w == 0 && r.score == 0);
    z = lobes({1500.3, 1845.9, 2191.5, 2537.1}, 100, 0.01);
    z[5] = std::nan("");
    hd::fsk4_comb_detect(z.data(), pl, 0, true, &r);
    CHECK(r.valid == 0 && r.w == 0);
    z[5] = -3.0;                                          // a negative sum quantises to 0
    hd::fsk4_comb_detect(z.data(), pl, 192, true, &r);
    CHECK(r.valid == 1);
    // the whole spectrum as the band, lobes at its ends: the windows and the refinement's +-w reach bins 0 and 4095 and no further
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 10.4 * BAUD, -FSD, FSD, pl) == HD_OK && pl.b_lo == 0 && pl.b_hi == 4095);
    hd::fsk4_comb_detect(lobes({32.0, 1375.0, 2719.0, 4063.0}, 60, 0.01).data(), pl, 192, true, &r);
    CHECK(r.valid == 1 && r.c0 >= 32 && r.c0 <= 64 && r.centroid_q8[3] <= 4095 * 256 && r.centroid_q8[0] >= 0);
    hd::fsk4_comb_detect(lobes({0.0, 1365.0, 2730.0, 4095.0}, 60, 0.01).data(), pl, 0, true, &r);
    CHECK(r.c0 >= 32 && r.c0 + ((3 * r.d + 2) >> 2) + 32 <= 4095);
    // the smallest window and a known spacing
    CHECK(hd::fsk4_comb_plan(FSD, 10.0, 50.0, 50.0, -100, 100, pl) == HD_OK && pl.w == 3 && pl.known == 1 && pl.d_lo == pl.d_hi);
    hd::fsk4_comb_detect(lobes({2040.0, 2046.4, 2052.8, 2059.2}, 2, 0.001).data(), pl, 0, true, &r);
    CHECK(r.spacing_q8 == (int32_t)(64 * pl.d_lo));
    // refusals
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 1.99 * BAUD, 3 * BAUD, -12000, 12000, pl) == HD_ERR_UNSUPPORTED);
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 3 * BAUD, -1000, 1000, pl) == HD_ERR_INVALID);
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 3 * BAUD, 1000, -1000, pl) == HD_ERR_INVALID);
    CHECK(hd::fsk4_comb_plan(FSD, std::nan(""), 2 * BAUD, 3 * BAUD, -12000, 12000, pl) == HD_ERR_INVALID);
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 1e300, -1e300, 1e300, pl) == HD_OK && pl.b_lo == 0 && pl.b_hi == 4095);
    CHECK(hd::fsk4_comb_plan(FSD, 8000.0, 16000.0, 16000.0, -FSD, FSD, pl) == HD_ERR_INVALID);       // a window as wide as an eighth of the spectrum
}

struct Run {
    std::vector<hd_fsk4_track_est> recs;
    std::vector<double> acc;
    std::vector<hd_fsk4_rx> rx;
    uint64_t retunes, late;
};

static Run run(const std::vector<float>& iq, size_t step, double f0_modem, bool reset_first)
{
    hd_fsk4_frame f;
    hd::fsk4_preset(HD_FSK4_HORUS_V1, &f);
    hd::Fsk4Stream m;
    hd_fsk4_params prm;
    hd::fsk4_params_default(&prm);
    m.set_params(prm);
    m.host_rings(4096);
    CHECK(hd::fsk4_tables(f, m.tab));
    CHECK(hd::fsk4_modem(m.s, FSD, BAUD, f0_modem, SP, 256) == HD_OK);
    hd::Fsk4TrackStream t;
    hd::fsk4_track_params_default(&t.prm);
    t.fsd = FSD;
    CHECK(hd::fsk4_comb_plan(FSD, BAUD, 2 * BAUD, 3.5 * BAUD, -9000, 9000, t.book.plan) == HD_OK);
    t.book.baud = BAUD; t.book.set = true;
    t.modem = &m;
    const size_t n = iq.size() / 2;
    if (reset_first) {                                    // some samples, a retune that waits, then a reset of both: nothing of it may stay
        t.push(iq.data(), std::min<size_t>(n, 12000));
        m.push_samples(iq.data(), 3000);
        uint32_t phi[4] = {1, 2, 3, 4};
        m.retune(phi, 1u << 30);
        t.reset(); m.reset();
        CHECK(hd::fsk4_modem(m.s, FSD, BAUD, f0_modem, SP, 256) == HD_OK);
    }
    for (size_t at = 0; at < n;) {
        const size_t k = std::min(n - at, step ? step : n);
        t.push(iq.data() + 2 * at, k);                   // the documented order: the tracker first
        for (size_t b = 0; b < k; b += 4096) {
            m.push_samples(iq.data() + 2 * (at + b), std::min<size_t>(4096, k - b));
            m.scan();
        }
        at += k;
    }
    Run r;
    r.recs.assign(t.book.log.begin(), t.book.log.end());
    r.acc = t.ts.acc;
    r.rx.assign(m.waiting.begin(), m.waiting.end());
    r.retunes = m.retunes; r.late = m.late;
    return r;
}

static void tracker()
{
    hd_fsk4_frame f;
    hd::fsk4_preset(HD_FSK4_HORUS_V1, &f);
    const size_t frames = 12, nsym = hd::fsk4_symbols(f.payload_bytes), n = frames * nsym * 32 + 8192;
    const double f0 = -4050.0, drift = 1500.0, two_pi = 6.283185307179586;
    std::normal_distribution<double> g(0.0, 0.6);
    std::vector<float> iq(2 * n);
    for (auto& v : iq) v = (float)g(rng);
    std::vector<std::vector<uint8_t>> payloads;
    double phase = 0;
    for (size_t k = 0; k < frames; ++k) {
        std::vector<uint8_t> p(f.payload_bytes);
        for (auto& b : p) b = (uint8_t)rng();
        const uint32_t crc = hd::fsk4_crc16(p.data(), p.size() - 2);
        p[p.size() - 2] = (uint8_t)crc; p[p.size() - 1] = (uint8_t)(crc >> 8);
        payloads.push_back(p);
        uint8_t bytes[2 + 64];
        CHECK(hd::fsk4_encode(f, p.data(), bytes) == nsym / 4);
        for (size_t sym = 0; sym < nsym; ++sym) {
            const size_t bit = 2 * sym;
            const uint32_t v = ((bytes[bit / 8] >> (7 - bit % 8)) & 1u) << 1 | ((bytes[(bit + 1) / 8] >> (7 - (bit + 1) % 8)) & 1u);
            for (size_t j = 0; j < 32; ++j) {
                const size_t i = (k * nsym + sym) * 32 + j;
                phase += two_pi * (f0 + SP * v + drift * (double)i / (double)n) / FSD;
                iq[2 * i] += (float)std::cos(phase); iq[2 * i + 1] += (float)std::sin(phase);
            }
        }
    }
    iq[2 * 40000] = std::nanf("");                        // one NaN sample: its segments' sums stay non-finite until the decay ... stays: records invalid from there on
    const Run poisoned = run(iq, 0, f0, false);
    CHECK(!poisoned.recs.empty() && poisoned.recs.back().rec.valid == 0 && poisoned.recs.front().rec.valid == 1);
    iq[2 * 40000] = 0.0f;
    const Run whole = run(iq, 0, f0, false);
    CHECK(whole.recs.size() == 9 && whole.retunes >= 3 && whole.late == 0);
    CHECK(whole.rx.size() == frames);
    for (size_t k = 0; k < std::min(frames, whole.rx.size()); ++k) CHECK(std::memcmp(whole.rx[k].payload, payloads[k].data(), f.payload_bytes) == 0);
    for (const auto& e : whole.recs) CHECK(e.rec.valid == 1 && e.end_sample == 2048u * (4u * (e.epoch + 1u) + 1u));
    const size_t steps[] = {1, 63, 64, 65, 4097};
    for (size_t step : steps) {
        const Run cut = run(iq, step, f0, step == 64);
        CHECK(cut.recs.size() == whole.recs.size() && cut.retunes == whole.retunes && cut.late == 0);
        CHECK(cut.recs.size() != whole.recs.size() || std::memcmp(cut.recs.data(), whole.recs.data(), cut.recs.size() * sizeof(hd_fsk4_track_est)) == 0);
        CHECK(cut.acc == whole.acc);
        CHECK(cut.rx.size() == whole.rx.size() && (cut.rx.empty() || std::memcmp(cut.rx.data(), whole.rx.data(), cut.rx.size() * sizeof(hd_fsk4_rx)) == 0));
    }
    const Run low = run(iq, 4097, f0 - BAUD, false);      // acquisition from a modem one baud low
    CHECK(low.rx.size() >= frames - 2 && low.retunes >= 1);
}

int main()
{
    detector();
    tracker();
    std::printf(failures ? "%d checks failed\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
