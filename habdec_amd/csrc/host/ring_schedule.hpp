// The tile schedule of the /32 stages' worker waves (kernels/stage1_ring.h: ring_worker) as pure functions: no HIP, no engine -- included by the
// kernels (every function is constexpr, so the device code runs the SAME arithmetic the host checks), by engine.cpp and by the stand-alone test
// program tests/ring_schedule_main.cpp.
//
// Rows.  A stream's push is `rows` rows of D samples (one output's stride); row r >= 0 is the call's r-th row, rows -hr .. -1 are the stage history.
// Output o is the sum over the rows o - hr .. o.  A tile is 64 loaded rows [row0, row0 + 64): lane l holds row row0 + l and ends up with output row0 + l.
//
// Plain schedule (the only one until the chained tiles came): every tile stands alone.  Its first hr lanes hold sums whose first rows lie in front of the
// tile -- thrown away -- so a tile stores 64 - hr outputs and consecutive tiles advance by that many rows; the last tile is pulled back to end with the
// call's last row (the outputs it shares with its neighbour are computed twice, identically).
//
// Chained schedule.  A RUN is walked by one wave, which keeps what leaves lane 63 at each of the hr hand-overs of a tile and feeds it into lane 0 at the
// same hand-over of the next one: the run's first tile stores 64 - hr outputs, every further tile starts 64 rows on and stores 64.  A stream is
// n_full runs of rl tiles (L = 64 rl - hr outputs each) and, where rows % L != 0, one closing run of the fewest tiles that cover the remainder, pulled
// back to end with the call's last row like the plain schedule's last tile.  (rl is cut to rows / 64 where a whole run would not fit the push: the
// stream is then one such run plus a closing tile.)  No run crosses a stream boundary, no tile loads a row past the push.
#pragma once
#include <stdint.h>

namespace hd {

struct RingTile {
    int32_t row0;            // first loaded row (-hr: a stream's first tile, whose first hr rows are the stage history)
    uint32_t out0, out_n;    // the outputs it stores: [out0, out0 + out_n)
    bool chained;            // lane 0 takes the previous tile's kept sums (that tile: index - 1, row0 - 64, same run)
    bool last;               // the stream's last tile (it carries the last T - 1 inputs into the next call's history)
};

struct RingSchedule {
    uint32_t rows = 0, hr = 0;
    uint32_t rl = 1;             // tiles of a full run (1: plain)
    uint32_t n_full = 0;         // chained: full runs
    uint32_t k_close = 0;        // chained: tiles of the closing run (0: none)
    uint32_t run_out = 0;        // chained: outputs of a full run, L = 64 rl - hr; plain: 64 - hr
    int32_t close_row0 = 0;      // chained: row0 of the closing run's first tile
    uint32_t nruns = 0;          // runs per stream (plain: = ntiles)
    uint32_t ntiles = 0;         // tiles per stream; 0: no schedule for these arguments
    bool chained = false;
};

// rows >= 64, 0 < hr < 32, run_len >= 1.  chained = false, or run_len < 2: the plain schedule.
constexpr RingSchedule ring_schedule(uint32_t rows, uint32_t hr, uint32_t run_len, bool chained)
{
    RingSchedule s{};
    if (rows < 64u || rows > (1u << 30) || hr == 0u || hr >= 32u || run_len == 0u || run_len > 4096u) return s;
    s.rows = rows; s.hr = hr;
    const uint32_t adv = 64u - hr;
    uint32_t rl = run_len < rows / 64u ? run_len : rows / 64u;
    if (!chained || rl < 2u) {
        s.rl = 1u; s.run_out = adv; s.ntiles = s.nruns = (rows + adv - 1u) / adv;
        return s;
    }
    s.chained = true; s.rl = rl; s.run_out = 64u * rl - hr;
    s.n_full = rows / s.run_out;                                  // >= 1: run_out <= rows
    const uint32_t rem = rows - s.n_full * s.run_out;
    s.k_close = rem ? (rem + hr + 63u) / 64u : 0u;                // 64 k - hr >= rem; <= rl because rem < run_out
    s.close_row0 = (int32_t)rows - (int32_t)(64u * s.k_close);    // (first output rows - (64 k - hr), first row hr in front of it)
    s.nruns = s.n_full + (s.k_close ? 1u : 0u);
    s.ntiles = s.n_full * rl + s.k_close;
    return s;
}

// run r < nruns of a stream: its tile count, the index of its first tile, that tile's row0
constexpr uint32_t ring_run_tiles(const RingSchedule& s, uint32_t r) { return s.chained ? (r < s.n_full ? s.rl : s.k_close) : 1u; }
constexpr uint32_t ring_run_first(const RingSchedule& s, uint32_t r) { return s.chained ? r * s.rl : r; }   // (the closing run is r = n_full)
constexpr int32_t ring_plain_row0(uint32_t rows, uint32_t hr, uint32_t tile)
{
    const uint32_t adv = 64u - hr, o = tile * adv < rows - adv ? tile * adv : rows - adv;
    return (int32_t)o - (int32_t)hr;
}
constexpr int32_t ring_run_row0(const RingSchedule& s, uint32_t r)
{
    if (!s.chained) return ring_plain_row0(s.rows, s.hr, r);
    return r < s.n_full ? (int32_t)(r * s.run_out) - (int32_t)s.hr : s.close_row0;
}

// tile k < ntiles of a stream
constexpr RingTile ring_tile(const RingSchedule& s, uint32_t k)
{
    RingTile t{};
    t.last = k + 1u == s.ntiles;
    if (!s.chained) {
        t.row0 = ring_plain_row0(s.rows, s.hr, k);
        t.out0 = (uint32_t)(t.row0 + (int32_t)s.hr); t.out_n = 64u - s.hr; t.chained = false;
        return t;
    }
    const uint32_t r = k < s.n_full * s.rl ? k / s.rl : s.n_full, j = k - r * s.rl;
    t.row0 = ring_run_row0(s, r) + (int32_t)(64u * j);
    t.chained = j != 0u;
    t.out0 = (uint32_t)(t.row0 + (int32_t)(t.chained ? 0u : s.hr)); t.out_n = t.chained ? 64u : 64u - s.hr;
    return t;
}

// ---- the ticket space of one XCD's share of a launch whose streams divide among the XCDs: `sx` streams per XCD, the first `sc` of them on the chained
// schedule -- one ticket per run, streams ascending --, the other sx - sc on the plain one, drawn tile by tile behind them (the guided hand-out: the end
// of a launch is ragged by one tile's time; single tiles cannot be chained).
struct RingTicket { uint32_t stream /* within the XCD's share */, tile /* index of the run's first tile in its stream's schedule */, ntiles; int32_t row0; bool plain; };
constexpr uint32_t ring_tickets(const RingSchedule& ch, const RingSchedule& pl, uint32_t sx, uint32_t sc) { return sc * ch.nruns + (sx - sc) * pl.ntiles; }
constexpr uint32_t ring_tiles_total(const RingSchedule& ch, const RingSchedule& pl, uint32_t sx, uint32_t sc) { return sc * ch.ntiles + (sx - sc) * pl.ntiles; }
constexpr RingTicket ring_ticket(const RingSchedule& ch, const RingSchedule& pl, uint32_t sc, uint32_t t)
{
    RingTicket k{};
    const uint32_t nch = sc * ch.nruns;
    if (t < nch) {
        k.stream = t / ch.nruns;
        const uint32_t r = t - k.stream * ch.nruns;
        k.tile = ring_run_first(ch, r); k.ntiles = ring_run_tiles(ch, r); k.row0 = ring_run_row0(ch, r); k.plain = false;
    } else {
        const uint32_t u = t - nch, sl = u / pl.ntiles;
        k.stream = sc + sl; k.tile = u - sl * pl.ntiles; k.ntiles = 1u; k.row0 = ring_plain_row0(pl.rows, pl.hr, k.tile); k.plain = true;
    }
    return k;
}
// streams of an XCD's share that keep the plain schedule for a guided hand-out of short_pct per cent
constexpr uint32_t ring_plain_streams(uint32_t sx, uint32_t short_pct) { return (uint32_t)(((uint64_t)sx * (short_pct > 100u ? 100u : short_pct) + 50u) / 100u); }

}  // namespace hd
