// Stand-alone check of habdec_amd/csrc/host/baud_probe.hpp and host/format_trial.hpp (built with -fsanitize=address,undefined and run by
// tests/test_baud_probe_host.py; its own main, no Python, no GPU).
// usage: baud_probe_asan FLOATS_FILE FSD BAUD_LO PUSH_SIZE [PUSH_SIZE ...]
// The file's float32 samples go through one probe stream in pushes of the given sizes, taken in turn, from buffers of exactly the push's size (so that
// a read past a push's end is a read past an allocation).  Prints sums of the state that the test compares with the library's, and the estimate.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "host/baud_probe.hpp"
#include "host/format_trial.hpp"

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: baud_probe_asan FLOATS_FILE FSD BAUD_LO PUSH_SIZE [PUSH_SIZE ...]\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<float> d;
    float buf[4096];
    for (size_t n; (n = std::fread(buf, sizeof(float), 4096, f)) > 0;) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    const double fsd = std::atof(argv[2]);
    hd_baud_probe_params prm;
    hd::baud_probe_params_default(&prm);
    prm.baud_lo = std::atof(argv[3]);
    if (!hd::baud_probe_params_ok(&prm, fsd)) { std::fprintf(stderr, "bad parameters\n"); return 2; }
    std::vector<size_t> sizes;
    for (int a = 4; a < argc; ++a) sizes.push_back((size_t)std::atol(argv[a]));
    auto t = std::make_unique<hd::BaudProbeTables>();
    t->make(fsd, prm);
    hd::BaudProbeStream s;
    size_t at = 0, turn = 0;
    while (at < d.size()) {
        const size_t n = std::min(std::max<size_t>(sizes[turn++ % sizes.size()], 1), d.size() - at);
        const std::vector<float> piece(d.begin() + at, d.begin() + at + n);
        s.push(*t, piece.data(), piece.size());
        at += n;
    }
    unsigned long long P = 0, Q = 0, NB = 0, N = 0, RE = 0, IM = 0, E = 0;
    for (const auto& c : s.c) { P += c.P; Q += c.Q; NB += c.NB; N += c.n; RE += (unsigned long long)(long long)c.re; IM += (unsigned long long)(long long)c.im; }
    for (const auto e : s.h.edges) E += e;
    hd_baud_estimate est;
    hd::baud_probe_estimate(*t, prm, s.h, s.c.data(), &est);
    std::printf("state %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.h.samples, E, P, Q, NB, N, RE, IM);
    std::printf("estimate %.17g %g %d %d\n", est.baud, est.nominal, est.settled, est.valid);

    // the framing trial on bits that frame now and then by chance (an LCG), pushed in uneven pieces
    hd::FormatTrial trial;
    std::vector<uint8_t> bits;
    uint32_t x = 12345;
    for (size_t pushes = 0; pushes < 200; ++pushes) {
        bits.resize(1 + x % 173);
        for (auto& b : bits) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 31); }
        trial.push_bits(bits.data(), bits.size());
    }
    hd_format_trial_result r;
    trial.get(&r);
    std::printf("trial %d\n", r.best);
    std::puts("baud_probe_asan OK");
    return 0;
}
