// Stand-alone check of the packed-IQ host code under AddressSanitizer / UBSan (tests/test_iq_formats_host.py builds and runs it; no GPU, no Python):
//   1. hd::iq_convert on buffers allocated at exactly n * bytes-per-sample bytes (and 2 n floats), every n in [0, 70) at every format -- a read or a
//      write one byte outside is the sanitizer's to report -- against the conversion table, code by code.
//   2. hd::IqFileBatch in packed mode over the files named on the command line, beside a cf32 batch over their converted twins, with a minimum take as
//      hd_ingest_run sets it: every round's counts, alive streams, rewinds and samples must agree, next_raw converted must equal next.
// usage: iq_formats_asan FMT CHUNK GRANULE LOOP MIN_TAKE ROUNDS packed0 cf32_0 [packed1 cf32_1 ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host/iq_file_batch.hpp"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); if (++fails > 20) std::exit(1); } } while (0)

static float table(int fmt, int code)
{
    if (fmt == HD_IQ_CS16) return (float)((double)code / 32768.0);
    if (fmt == HD_IQ_CS8) return (float)((double)code / 128.0);
    return (float)((2.0 * code - 255.0) / 256.0);
}

static void check_convert()
{
    for (int fmt : {HD_IQ_CS16, HD_IQ_CS8, HD_IQ_CU8}) {
        const size_t bps = hd::iq_bytes(fmt);
        for (size_t n = 0; n < 70; ++n) {
            std::unique_ptr<unsigned char[]> src(new unsigned char[n * bps]);      // exactly the bytes the conversion may read
            std::unique_ptr<float[]> out(new float[2 * n]);
            for (size_t i = 0; i < n * bps; ++i) src[i] = (unsigned char)(i * 37u + n * 11u + 0x80u);
            hd::iq_convert(fmt, src.get(), n, out.get());
            for (size_t i = 0; i < 2 * n; ++i) {
                int code;
                if (fmt == HD_IQ_CS16) code = (int16_t)(uint16_t)(src[2 * i] | (src[2 * i + 1] << 8));
                else if (fmt == HD_IQ_CS8) code = (int8_t)src[i];
                else code = src[i];
                CHECK(out[i] == table(fmt, code), "convert fmt %d n %zu i %zu: %g != %g", fmt, n, i, (double)out[i], (double)table(fmt, code));
            }
        }
    }
    CHECK(hd::iq_bytes(HD_IQ_CF32) == 8 && hd::iq_bytes(HD_IQ_CS16) == 4 && hd::iq_bytes(HD_IQ_CS8) == 2 && hd::iq_bytes(HD_IQ_CU8) == 2, "iq_bytes");
    CHECK(hd::iq_bytes(4) == 0 && hd::iq_bytes(-1) == 0, "iq_bytes of an unknown format");
}

int main(int argc, char** argv)
{
    check_convert();
    if (argc >= 9 && (argc - 7) % 2 == 0) {
        const int fmt = std::atoi(argv[1]);
        const uint32_t chunk = (uint32_t)std::atoi(argv[2]), granule = (uint32_t)std::atoi(argv[3]), min_take = (uint32_t)std::atoi(argv[5]);
        const bool loop = std::atoi(argv[4]) != 0;
        const int rounds = std::atoi(argv[6]);
        std::vector<std::string> packed, plain;
        for (int i = 7; i < argc; i += 2) { packed.push_back(argv[i]); plain.push_back(argv[i + 1]); }
        const size_t S = packed.size(), bps = hd::iq_bytes(fmt);
        hd::IqFileBatch a, b, c;
        CHECK(a.open(packed, loop, chunk, granule, 0.0, fmt) && b.open(plain, loop, chunk, granule) && c.open(packed, loop, chunk, granule, 0.0, fmt), "open");
        CHECK(!hd::IqFileBatch().open(packed, loop, chunk, granule, 0.0, 7), "an unknown format must not open");
        a.set_min_take(min_take); b.set_min_take(min_take); c.set_min_take(min_take);
        for (size_t s = 0; s < S; ++s) CHECK(a.file((uint32_t)s).count() == b.file((uint32_t)s).count(), "count of stream %zu", s);
        // slabs at exactly the size a round may fill (stride = chunk)
        std::unique_ptr<float[]> fa(new float[S * chunk * 2]), fb(new float[S * chunk * 2]), fc(new float[S * chunk * 2]);
        std::unique_ptr<unsigned char[]> raw(new unsigned char[S * chunk * bps]);
        std::vector<uint32_t> na(S), nb(S), nc(S);
        for (int r = 0; r < rounds; ++r) {
            const uint32_t alive_a = a.next(fa.get(), chunk, na.data()), alive_b = b.next(fb.get(), chunk, nb.data());
            const uint32_t alive_c = c.next_raw(raw.get(), chunk, nc.data());
            CHECK(alive_a == alive_b && alive_a == alive_c, "round %d: alive %u %u %u", r, alive_a, alive_b, alive_c);
            for (size_t s = 0; s < S; ++s) {
                CHECK(na[s] == nb[s] && na[s] == nc[s], "round %d stream %zu: n %u %u %u", r, s, na[s], nb[s], nc[s]);
                CHECK(na[s] % granule == 0 && na[s] <= chunk, "round %d stream %zu: n %u", r, s, na[s]);
                CHECK(a.file((uint32_t)s).rewinds() == b.file((uint32_t)s).rewinds(), "round %d stream %zu: rewinds", r, s);
                hd::iq_convert(fmt, raw.get() + s * chunk * bps, nc[s], fc.get() + s * chunk * 2);
                CHECK(!std::memcmp(fa.get() + s * chunk * 2, fb.get() + s * chunk * 2, (size_t)na[s] * 8), "round %d stream %zu: packed next != cf32 next", r, s);
                CHECK(!std::memcmp(fa.get() + s * chunk * 2, fc.get() + s * chunk * 2, (size_t)na[s] * 8), "round %d stream %zu: next_raw converted != next", r, s);
            }
        }
    } else if (argc != 1) {
        std::fprintf(stderr, "usage: iq_formats_asan FMT CHUNK GRANULE LOOP MIN_TAKE ROUNDS packed0 cf32_0 [packed1 cf32_1 ...]\n");
        return 2;
    }
    if (fails) return 1;
    std::puts("iq_formats_asan OK");
    return 0;
}
