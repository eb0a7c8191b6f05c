// Stand-alone check of habdec_amd/csrc/host/ring_schedule.hpp (built with -fsanitize=address,undefined and run by tests/test_ring_schedule.py).
//  1. the schedule's properties, for rows x HR x run_len x {chained, plain};
//  2. the ticket space of an XCD's share: every (stream, tile) of the share handed out exactly once, runs whole, inside one stream;
//  3. a float32 emulation of the worker wave's systolic tap loop with the chained hand-over (lane 0 takes what left lane 63 at the same hand-over of
//     the tile before), against plain left-to-right sums: bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../habdec_amd/csrc/host/ring_schedule.hpp"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void check_schedule(uint32_t rows, uint32_t hr, uint32_t run_len, bool chained)
{
    const hd::RingSchedule s = hd::ring_schedule(rows, hr, run_len, chained);
    CHECK(s.ntiles > 0, "rows %u hr %u rl %u ch %d", rows, hr, run_len, (int)chained);
    if (!s.ntiles) return;
    std::vector<uint32_t> cover(rows, 0);
    std::vector<hd::RingTile> tiles;
    for (uint32_t k = 0; k < s.ntiles; ++k) tiles.push_back(hd::ring_tile(s, k));
    for (uint32_t k = 0; k < s.ntiles; ++k) {
        const hd::RingTile& t = tiles[k];
        // no tile loads rows beyond `rows`; rows in front of the push only as the stage history of the stream's first tile
        CHECK(t.row0 + 64 <= (int32_t)rows, "tile %u row0 %d rows %u", k, t.row0, rows);
        CHECK(t.row0 >= 0 || (k == 0 && t.row0 == -(int32_t)hr), "tile %u row0 %d", k, t.row0);
        // lane l holds output row0 + l; a tile that is not chained cannot store its first hr lanes
        CHECK(t.out0 == (uint32_t)(t.row0 + (int32_t)(t.chained ? 0u : hr)) && t.out_n == (t.chained ? 64u : 64u - hr), "tile %u", k);
        CHECK(t.out0 + t.out_n <= rows, "tile %u stores past the push", k);
        for (uint32_t o = t.out0; o < t.out0 + t.out_n && o < rows; ++o) ++cover[o];
        // a chained tile's predecessor is the tile 64 rows before it, in the same run
        if (t.chained) {
            CHECK(k > 0 && tiles[k - 1].row0 + 64 == t.row0, "tile %u row0 %d", k, t.row0);
            CHECK(chained, "a chained tile in the plain schedule");
        }
        CHECK(t.last == (k + 1 == s.ntiles), "tile %u", k);
    }
    for (uint32_t o = 0; o < rows; ++o) CHECK(cover[o] >= 1, "output %u not covered (rows %u hr %u rl %u ch %d)", o, rows, hr, run_len, (int)chained);
    // runs: consecutive tile indices, the first one not chained, the others chained; together they are the stream's tiles
    uint32_t next = 0;
    for (uint32_t r = 0; r < s.nruns; ++r) {
        const uint32_t f = hd::ring_run_first(s, r), n = hd::ring_run_tiles(s, r);
        CHECK(f == next && n >= 1 && n <= (run_len ? run_len : 1u), "run %u first %u n %u", r, f, n);
        CHECK(f + n <= s.ntiles, "run %u leaves the stream", r);
        if (f + n > s.ntiles) return;
        CHECK(tiles[f].row0 == hd::ring_run_row0(s, r) && !tiles[f].chained, "run %u", r);
        for (uint32_t j = 1; j < n; ++j) CHECK(tiles[f + j].chained, "run %u tile %u", r, j);
        next = f + n;
    }
    CHECK(next == s.ntiles, "runs cover %u of %u tiles", next, s.ntiles);
    if (!chained) {
        const uint32_t adv = 64u - hr;
        CHECK(s.ntiles == (rows + adv - 1u) / adv && s.nruns == s.ntiles, "plain tile count");
        for (uint32_t k = 0; k < s.ntiles; ++k) CHECK(tiles[k].out0 == (k * adv < rows - adv ? k * adv : rows - adv), "plain tile %u", k);
    } else if (s.chained) {
        const uint32_t L = 64u * s.rl - hr;
        CHECK(s.n_full == rows / L && s.nruns == s.n_full + (rows % L ? 1u : 0u), "run count");
        if (run_len <= rows / 64u) CHECK(s.rl == run_len, "run length");
    }
}

static void check_tickets(uint32_t rows, uint32_t hr, uint32_t run_len, uint32_t sx, uint32_t sc)
{
    const hd::RingSchedule ch = hd::ring_schedule(rows, hr, run_len, true), pl = hd::ring_schedule(rows, hr, 1u, false);
    const uint32_t n = hd::ring_tickets(ch, pl, sx, sc);
    std::vector<std::vector<uint32_t>> seen(sx);
    for (uint32_t s = 0; s < sx; ++s) seen[s].assign(s < sc ? ch.ntiles : pl.ntiles, 0);    // tiles per stream: the same for all streams of a mode
    uint32_t tiles = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const hd::RingTicket k = hd::ring_ticket(ch, pl, sc, t);
        CHECK(k.stream < sx && k.plain == (k.stream >= sc) && k.ntiles >= 1, "ticket %u", t);
        if (k.stream >= sx) return;
        const hd::RingSchedule& s = k.plain ? pl : ch;
        CHECK(k.tile + k.ntiles <= s.ntiles, "ticket %u crosses its stream's end", t);
        if (k.tile + k.ntiles > s.ntiles) return;
        CHECK(hd::ring_tile(s, k.tile).row0 == k.row0 && !hd::ring_tile(s, k.tile).chained, "ticket %u", t);
        for (uint32_t j = 0; j < k.ntiles; ++j) {
            ++seen[k.stream][k.tile + j]; ++tiles;
            const hd::RingTile tl = hd::ring_tile(s, k.tile + j);
            CHECK(tl.row0 == k.row0 + (int32_t)(64u * j) && tl.chained == (j != 0), "ticket %u tile %u", t, j);   // what the worker wave walks: +64 rows per tile
        }
    }
    CHECK(tiles == hd::ring_tiles_total(ch, pl, sx, sc), "tiles %u", tiles);
    for (uint32_t s = 0; s < sx; ++s) for (size_t k = 0; k < seen[s].size(); ++k) CHECK(seen[s][k] == 1, "stream %u tile %zu handed out %u times", s, k, seen[s][k]);
}

// ---- the tap loop, emulated.  T taps, rows of 32 samples, HR = ceil((T - 1) / 32) halo rows; slot JS of a lane's first row carries tap 0.
// Reference: out[o] = sum_t x[32 o - (T - 1) + t] * tap[t], one float accumulator, ascending t, multiply and add rounded separately.
static float mul_add(float acc, float x, float k) { volatile float p = x * k; return acc + p; }     // (no contraction into a fused multiply-add)

static void check_handover(uint32_t rows, int T, uint32_t run_len, uint32_t seed)
{
    const int HR = (T - 1 + 31) / 32, JS = HR * 32 - (T - 1), NS = JS + T;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> d(-1.f, 1.f);
    std::vector<float> ext((size_t)(rows + HR) * 32), tap(T);                 // history-extended samples: row -HR is ext row 0
    for (auto& v : ext) v = d(rng);
    for (auto& v : tap) v = d(rng) * 0.1f;
    auto row = [&](int32_t r) { return ext.data() + (size_t)(r + HR) * 32; };
    std::vector<float> ref(rows), got(rows);
    for (uint32_t o = 0; o < rows; ++o) {
        float acc = 0.f;
        const float* w = row((int32_t)o - HR) + JS;                           // the window: T samples from slot JS of row o - HR
        for (int t = 0; t < T; ++t) acc = mul_add(acc, w[t], tap[t]);
        ref[o] = acc;
    }
    const hd::RingSchedule s = hd::ring_schedule(rows, (uint32_t)HR, run_len, true);
    uint32_t nan_bits = 0x7FC00000u; float poison; std::memcpy(&poison, &nan_bits, 4);
    for (auto& v : got) v = poison;
    std::vector<float> keep(HR, poison);                                       // one wave walks the stream's tiles in order (any wave, any order of RUNS, gives the same)
    for (uint32_t k = 0; k < s.ntiles; ++k) {
        const hd::RingTile t = hd::ring_tile(s, k);
        if (!t.chained) for (auto& v : keep) v = poison;                       // (another wave's leftovers: whatever they are, they must not reach a stored lane)
        float acc[64];
        for (int l = 0; l < 64; ++l) acc[l] = 0.f;
        for (int step = 0; step <= HR; ++step) {                               // step `step`: slots [32 step, 32 step + 32) of the slot sequence on the lane's own row
            for (int l = 0; l < 64; ++l) {
                const float* x = row(t.row0 + l);
                for (int j = 0; j < 32; ++j) { const int slot = 32 * step + j; if (slot >= JS && slot < NS) acc[l] = mul_add(acc[l], x[j], tap[slot - JS]); }
            }
            if (step < HR) {                                                   // hand-over number `step`
                const float out63 = acc[63];
                for (int l = 63; l > 0; --l) acc[l] = acc[l - 1];
                acc[0] = keep[step];
                keep[step] = out63;
            }
        }
        for (uint32_t l = t.chained ? 0u : (uint32_t)HR; l < 64u; ++l) got[(uint32_t)(t.row0 + (int32_t)l)] = acc[l];
    }
    for (uint32_t o = 0; o < rows; ++o) {
        uint32_t a, b; std::memcpy(&a, &ref[o], 4); std::memcpy(&b, &got[o], 4);
        CHECK(a == b, "output %u: %08x against %08x (rows %u T %d rl %u)", o, b, a, rows, T, run_len);
    }
}

// With arguments (rows hr run_len chained) the program prints that schedule instead -- one line per tile: k row0 out0 out_n chained last first_of_run --
// for tests that need the tile geometry (tests/fir_probe.py: which outputs are wrapped rows, a run's first tile, the closing tile).
static int print_schedule(char** a)
{
    const hd::RingSchedule s = hd::ring_schedule((uint32_t)std::strtoul(a[1], nullptr, 10), (uint32_t)std::strtoul(a[2], nullptr, 10), (uint32_t)std::strtoul(a[3], nullptr, 10), std::strtoul(a[4], nullptr, 10) != 0);
    for (uint32_t k = 0; k < s.ntiles; ++k) {
        const hd::RingTile t = hd::ring_tile(s, k);
        std::printf("tile %u %d %u %u %d %d %d\n", k, t.row0, t.out0, t.out_n, (int)t.chained, (int)t.last, (int)!t.chained);
    }
    return s.ntiles ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 5) return print_schedule(argv);
    const uint32_t rows_set[] = {64, 128, 192, 2048, 32768}, hr_set[] = {6, 7}, rl_set[] = {2, 3, 4, 9};
    for (uint32_t rows : rows_set) for (uint32_t hr : hr_set) for (uint32_t rl : rl_set) for (int ch = 0; ch < 2; ++ch) check_schedule(rows, hr, rl, ch != 0);
    // the figure the design quotes: /32, 2048 rows, runs of four -> 8 x 4 + 1 = 33 tiles against 36
    CHECK(hd::ring_schedule(2048, 7, 4, true).ntiles == 33 && hd::ring_schedule(2048, 7, 4, false).ntiles == 36, "tiles per 65536-sample push");
    CHECK(hd::ring_schedule(63, 7, 4, true).ntiles == 0 && hd::ring_schedule(64, 0, 4, true).ntiles == 0, "arguments without a schedule");
    for (uint32_t rows : rows_set) for (uint32_t hr : hr_set) for (uint32_t rl : rl_set) {
        if (rows > 2048) continue;
        for (uint32_t pct : {0u, 25u, 100u}) for (uint32_t sx : {1u, 8u, 32u}) check_tickets(rows, hr, rl, sx, sx - hd::ring_plain_streams(sx, pct));
    }
    CHECK(hd::ring_plain_streams(8, 25) == 2 && hd::ring_plain_streams(128, 25) == 32 && hd::ring_plain_streams(8, 0) == 0 && hd::ring_plain_streams(8, 100) == 8, "plain streams");
    uint32_t seed = 1;
    for (uint32_t rows : {64u, 128u, 192u, 2048u}) for (int T : {212, 174}) for (uint32_t rl : rl_set) check_handover(rows, T, rl, seed++);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ring schedule: all checks passed\n");
    return 0;
}
