// The SSDV receiver's host restatement (habdec_amd/csrc/host/ssdv.hpp) run stand-alone, for AddressSanitizer and UBSan on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I habdec_amd/csrc -I include tools/ssdv_host_check.cpp -o /tmp/ssdv_host_check
//   /tmp/ssdv_host_check tests/golden
//
// It walks the shapes of the tests' case table (sizes, offsets, errors up to and past the code's reach, erasures, the sync byte, no-FEC, zeros,
// back-to-back packets, noise; pushes of 1, 255, 256, 257 and 4097 bytes; a reset), a synthetic row of records with lost characters through the gap
// rule and -- given the directory of the golden files -- one row of the tests' ladder (seed 3, sigma 0.28: the clocked restatement's records, written
// by tools/gen_golden_ssdv.py), and checks the outcomes it knows.  Exit status 0: every check held and no sanitizer spoke.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "host/ssdv.hpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static std::mt19937 rng(12345);
static std::vector<uint8_t> rnd(size_t n) { std::vector<uint8_t> v(n); for (auto& b : v) b = (uint8_t)rng(); return v; }

struct Result { std::vector<hd_ssdv_packet> pk; hd_ssdv_counters st; };

static Result run(const std::vector<uint8_t>& b, const std::vector<uint32_t>* c, size_t cut, bool behind_reset = false)
{
    hd::SsdvStream s;
    if (behind_reset) { const auto junk = rnd(300); s.push_bytes(junk.data(), nullptr, junk.size()); s.scan(); s.out.clear(); s.reset(); }
    for (size_t at = 0; at < b.size(); at += cut) {
        const size_t k = std::min(cut, b.size() - at);
        s.push_bytes(b.data() + at, c ? c->data() + at : nullptr, k);
        s.scan();
    }
    Result r;
    r.pk.assign(s.out.begin(), s.out.end());
    s.stats(&r.st);
    return r;
}

static bool same(const Result& a, const Result& b)
{
    if (a.pk.size() != b.pk.size() || std::memcmp(&a.st, &b.st, sizeof a.st)) return false;
    for (size_t i = 0; i < a.pk.size(); ++i) if (std::memcmp(&a.pk[i], &b.pk[i], sizeof a.pk[i])) return false;
    return true;
}

// every cut and the reset give what one push gives
static Result all_cuts(const std::vector<uint8_t>& b, const std::vector<uint32_t>* c = nullptr)
{
    const Result one = run(b, c, b.size() ? b.size() : 1);
    for (size_t cut : {1u, 255u, 256u, 257u, 4097u}) CHECK(same(run(b, c, cut), one));
    CHECK(same(run(b, c, b.size() ? b.size() : 1, true), one));
    return one;
}

int main(int argc, char** argv)
{
    uint8_t P[256], N[256];
    const auto pay = rnd(205);
    hd::ssdv_make_packet(0x66, "TEST01", 3, 0x0102, 320, 240, 4, 7, 0x0304, pay.data(), P);
    hd::ssdv_make_packet(HD_SSDV_TYPE_NOFEC, "NOFEC", 9, 1, 160, 128, 0, 0, 0, pay.data(), N);
    uint8_t syn[32];
    CHECK(hd::ssdv_syndromes(P, syn));
    const std::vector<uint8_t> pkt(P, P + 256);

    CHECK(all_cuts(rnd(255)).st.decided == 0);
    {
        const Result r = all_cuts(pkt);
        CHECK(r.st.decided == 1 && r.pk.size() == 1 && r.pk[0].trial == 0 && r.pk[0].packet_id == 0x0102 && !std::strcmp(r.pk[0].callsign, "TEST01"));
    }
    for (size_t o : {0u, 1u, 63u, 64u, 255u, 256u, 257u}) {
        auto b = rnd(o);
        b.insert(b.end(), pkt.begin(), pkt.end());
        const auto tail = rnd(40);
        b.insert(b.end(), tail.begin(), tail.end());
        const Result r = all_cuts(b);
        CHECK(r.pk.size() == 1 && r.pk[0].pos == o && !std::memcmp(r.pk[0].data, P, 256));
    }
    auto hit = [&](std::vector<uint8_t> b, std::initializer_list<int> at) { int k = 0; for (int j : at) b[j] ^= (uint8_t)(1 + 37 * k++); return b; };
    auto hit_n = [&](int n) { std::vector<uint8_t> b = pkt; for (int k = 0; k < n; ++k) b[2 + 9 * k] ^= (uint8_t)(1 + 37 * k); return b; };
    for (int n : {1, 15, 16}) { const Result r = all_cuts(hit_n(n)); CHECK(r.pk.size() == 1 && r.pk[0].errors == (uint32_t)n && r.pk[0].trial == 0); }
    CHECK(all_cuts(hit_n(17)).pk.empty());
    {
        std::vector<uint32_t> c(256, hd::kSsdvConfMax);
        for (int k = 0; k < 17; ++k) c[2 + 9 * k] = 10 + k;
        const Result r = all_cuts(hit_n(17), &c);
        CHECK(r.pk.size() == 1 && r.pk[0].trial == 1 && r.pk[0].errors == 9 && r.pk[0].erasures == 8 && r.pk[0].erasures_changed == 8);
    }
    {
        std::vector<uint32_t> c(256, hd::kSsdvConfMax);
        for (int k = 0; k < 24; ++k) c[2 + 9 * k] = 10 + k;
        Result r = all_cuts(hit(hit_n(24), {240, 241, 250, 255}), &c);
        CHECK(r.pk.size() == 1 && r.pk[0].trial == 3 && r.pk[0].errors == 4 && r.pk[0].erasures_changed == 24 && !std::memcmp(r.pk[0].data, P, 256));
        CHECK(all_cuts(hit(hit_n(24), {240, 241, 250, 255, 1}), &c).pk.empty());
        r = all_cuts(hit(pkt, {230, 231, 232, 233}), &c);
        CHECK(r.pk.size() == 1 && r.pk[0].trial == 0 && r.pk[0].errors == 4 && r.pk[0].erasures_changed == 0);
    }
    for (int j : {1, 223, 224, 255}) { const Result r = all_cuts(hit(pkt, {j})); CHECK(r.pk.size() == 1 && r.pk[0].errors == 1); }
    { const Result r = all_cuts(hit(pkt, {0})); CHECK(r.pk.size() == 1 && r.pk[0].data[0] == 0x55 && r.pk[0].errors == 0); }
    {
        const std::vector<uint8_t> nf(N, N + 256);
        const Result r = all_cuts(nf);
        CHECK(r.pk.size() == 1 && r.pk[0].trial == HD_SSDV_NOFEC && r.st.packets[4] == 1);
        CHECK(all_cuts(hit(nf, {100})).pk.empty());
    }
    { const Result r = all_cuts(std::vector<uint8_t>(600, 0)); CHECK(r.pk.empty() && r.st.crc_bad == 4 * 345); }
    {
        std::vector<uint8_t> b = pkt;
        b.insert(b.end(), pkt.begin(), pkt.end());
        const Result r = all_cuts(b);
        CHECK(r.pk.size() == 2 && r.pk[1].pos == 256);
    }
    CHECK(all_cuts(rnd(4096)).pk.empty());

    // records with lost characters, soft values from a noisy row's statistics, through the gap rule in pushes of 100 records
    {
        std::vector<hd_clocked_record> rec;
        std::normal_distribution<double> g(0.0, 1.0);
        uint64_t pos = 4000;
        std::vector<uint8_t> sent;
        for (int k = 0; k < 3; ++k) {
            uint8_t q[256];
            const auto pl = rnd(205);
            hd::ssdv_make_packet(0x66, "LADDER", 1, (uint16_t)k, 320, 240, 0, 0, (uint16_t)(5 * k), pl.data(), q);
            sent.insert(sent.end(), q, q + 256);
        }
        for (size_t i = 0; i < sent.size(); ++i, pos += 293) {
            if (i % 97 == 50) continue;                              // a lost character
            hd_clocked_record r;
            std::memset(&r, 0, sizeof r);
            r.pos = pos + (uint64_t)(rng() % 21);
            for (int b = 0; b < 8; ++b) {
                const int bit = (sent[i] >> b) & 1;
                const double v = (bit ? 1.0 : -1.0) * 9000.0 + 3300.0 * g(rng);
                r.data[b] = (int32_t)v;
                r.ch |= (uint32_t)(v > 0) << b;
            }
            rec.push_back(r);
        }
        hd::SsdvStream s, plain;
        for (size_t at = 0; at < rec.size(); at += 100) { s.push_records(rec.data() + at, std::min<size_t>(100, rec.size() - at), 293); s.scan(); }
        plain.push_records(rec.data(), rec.size(), 0);
        plain.scan();
        std::printf("records %zu: gap rule delivers %zu of 3 (fillers %llu), without it %zu\n", rec.size(), s.out.size(), (unsigned long long)s.fillers, plain.out.size());
        CHECK(s.fillers == 8 && s.out.size() >= plain.out.size() && s.out.size() >= 2);
        for (const auto& p : s.out) CHECK(!std::memcmp(p.data, sent.data() + 256 * p.packet_id, 256));
    }
    // one row of the ladder: the clocked restatement's records of seed 3 at sigma 0.28 (tests/golden, written by tools/gen_golden_ssdv.py)
    if (argc > 1) {
        auto slurp = [&](const char* name) {
            std::vector<uint8_t> v;
            const std::string path = std::string(argv[1]) + "/" + name;
            if (FILE* f = std::fopen(path.c_str(), "rb")) {
                uint8_t buf[4096];
                for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
                std::fclose(f);
            }
            return v;
        };
        const auto raw = slurp("ssdv_ladder_s3_028.records"), sent = slurp("ssdv_ladder_s3_028.packets");
        CHECK(!raw.empty() && raw.size() % sizeof(hd_clocked_record) == 0 && sent.size() == 6 * 256);
        std::vector<hd_clocked_record> rec(raw.size() / sizeof(hd_clocked_record));
        std::memcpy(rec.data(), raw.data(), rec.size() * sizeof(hd_clocked_record));
        hd::SsdvStream all, plain;
        for (size_t at = 0; at < rec.size(); at += 37) { all.push_records(rec.data() + at, std::min<size_t>(37, rec.size() - at), 293); all.scan(); }
        plain.push_records(rec.data(), rec.size(), 0);
        plain.scan();
        size_t plain0 = 0;
        for (const auto& p : plain.out) plain0 += p.trial == 0;
        std::printf("ladder row, %zu records: all trials with the gap rule %zu of 6 (fillers %llu, crc_bad %llu), trial 0 without it %zu\n", rec.size(), all.out.size(),
                    (unsigned long long)all.fillers, (unsigned long long)all.crc_bad, plain0);
        CHECK(all.out.size() == 5 && all.out.size() >= plain0 + 3);      // (what the GPU test's stream 0 delivers: positions 255, 511, 767, 1023, 1279)
        for (const auto& p : all.out) CHECK(p.packet_id < 6 && !std::memcmp(p.data, sent.data() + 256 * p.packet_id, 256));
    }
    std::printf(failures ? "%d checks FAILED\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
