"""Sparse probes and a float64 model for the FIR stages of the chain (the decimators, the low-pass): a COMPONENTWISE check of the fast arithmetic mode.

The norm-wise 1e-5 gate of tests/test_gpu_fast.py is relative to the output's peak; the edge taps of the 212-tap table are 4e-6 .. 1.3e-5 of the centre
tap, so a wrong, skipped or doubled edge tap, a wrapped sum that lost one of its two chains, or a history row off by one at the far end of the window
passes it.  On input that is zero except for isolated samples of power-of-two amplitude, float32 arithmetic is nearly exact: a first-stage output has at
most one non-zero term and equals amplitude x tap exactly, in either mode and in any summation order; a second-stage output has a handful of terms.

The bound (model()).  For one output, a sum of products k[t] * x[t] of which m have x[t] != 0 (as far as the model can tell: x[t] != 0 or e_in[t] != 0):

    e_out = gamma(m) * sum_t |k[t]| (|x[t]| + e_in[t])  +  sum_t |k[t]| e_in[t],      gamma(m) = m u / (1 - m u),   u = 2^-24

where e_in bounds what the kernel's input may differ from the model's.  It is DERIVED, not measured: any summation tree over m non-zero leaves -- with
separately rounded products and sums, or with fused multiply-add -- puts at most m roundings on the path of a term (one for its product, at most m - 1
sums), which is the classical gamma(m) of Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a product with an exact zero is an exact
zero and adding it is exact, so zero terms neither count nor disturb.  It therefore covers the oracle's sequential loop, the kernels' two-chain loops and
the sums wrapped from one tile into the next alike, and needs no margin.  Where every product is exact (the probe's samples are +-1, +-0.5: first
stage) a term's path holds one rounding less: gamma(m - 1), so a lone term has bound 0 and must match bit for bit.  Real and imaginary parts are two
independent real filters (the taps are real): everything here is per component.

The model restates the oracle's framing (oracle/habdec_oracle.cpp: orc_decimator_run, orc_fir_run, orc_decoder_process_body): zero history at a stream's
start, a decimator's next history read from the caller's buffer AFTER its head was overwritten with the outputs, the low-pass fed in batches of 256."""
import numpy as np

U = 2.0 ** -24
AMPS = np.array([1, -1, 0.5, -0.5, 1j, -1j, 0.5j, -0.5j], np.complex64)
LP_BATCH = 256


def gamma(m):
    m = np.maximum(np.asarray(m, np.float64), 0.0)
    return m * U / (1.0 - m * U)


def tables(factor):
    """[(ratio, float32 taps)] of a total factor: the oracle's tables (tests/test_host_logic.py pins the host library's against the same)."""
    from oracle import pyoracle
    O = pyoracle.Stages("oracle")
    return [(r, O.decim_taps(name, r)) for r, name in O.decim_plan(factor)]


def total_ratio(stages):
    return int(np.prod([r for r, _ in stages]))


def min_spacing(stages, lowpass_ntaps=0):
    """Input samples between impulses so that no window of the last decimation stage (of the low-pass, if given) sees two of them."""
    sp, rate = 0, 1
    for r, k in stages:
        sp += rate * (len(k) - 1)
        rate *= r
    sp += rate * max(lowpass_ntaps - 1, 0)
    return sp + 1


def spacing_for(stages, lowpass_ntaps=0):
    """The least odd spacing >= min_spacing: consecutive impulses step the decimation phase by an odd amount, so a run of them visits every residue
    modulo the (power of two) total ratio, and hardly an output between two impulses is left without a term."""
    return min_spacing(stages, lowpass_ntaps) | 1


def boundary_deltas(stages):
    """Distances (impulse in front of a push boundary) that between them put every tap index of every stage into a window that spans two pushes: 1 .. R1
    (the top tap of each residue class of the first stage; the taps below follow from the later outputs), and one far enough back for the last R2 first-stage
    outputs of the push to be non-zero (every residue class of the second stage's history)."""
    R1, T1 = stages[0][0], len(stages[0][1])
    d = list(range(1, R1 + 1))
    if len(stages) == 2:
        far = stages[1][0] * R1 + 1
        assert far <= R1 + T1 - 1
        d.append(far)
    return d


def boundary_designs(stages):
    """Every distance of boundary_deltas() once for the real and once for the imaginary part: the two are independent filters on the two halves of a
    float2, so each has to meet the history carry on its own."""
    return [(d, comp) for comp in (0, 1) for d in boundary_deltas(stages)]


def designing_streams(S, stages):
    """How many of a case's streams design boundaries: no more than there are distances, so that where streams are many the rest keep a layout of
    their own (other rows of a tile) and a designing stream takes its distance through both parts."""
    return min(S, len(boundary_deltas(stages)))


def calls_needed(S, stages, every=1):
    """Calls after which every entry of boundary_designs() has had its boundary, whichever boundary each stream designs first."""
    return every * -(-len(boundary_designs(stages)) // designing_streams(S, stages)) + 1


def probe_positions(n_calls, C, S, stages, every=1, shift=77, spread=4):
    """(positions, forced): per stream the sorted impulse positions in [0, n_calls * C), no two closer than min_spacing(), and {position: 0 | 1} of the
    impulses that must be real or imaginary.  Stream s DESIGNS every `every`-th push boundary: one impulse in front of it, at a distance and in the
    part that boundary_designs() names, walking through them over streams and boundaries.  Between two designed impulses the
    others follow at spacing_for() and the last gap takes what is left; in front of the first and behind the last they follow at spacing_for().  Of
    its first `every` boundaries stream s designs first the one that leaves the (s % spread)-th shortest empty stretch at its start (the shortest for
    all would put every stream's impulses into the same rows of a tile).  Streams beyond designing_streams() design no
    boundary and start s * shift (modulo an eighth of the spacing) in: other rows of a tile than the designed streams'."""
    P, lo, N = spacing_for(stages), min_spacing(stages), n_calls * C
    deltas, D = boundary_designs(stages), designing_streams(S, stages)
    out, forced = [], []
    for s in range(S):
        cand = [b for b in range(1, min(every, n_calls - 1) + 1)] if s < D else []
        delta = lambda j: deltas[(j * D + s) % len(deltas)][0]
        b0 = sorted(cand, key=lambda b: (b * C - delta(0)) % P)[min(s % spread, len(cand) - 1)] if cand else None
        fixed = [b * C - delta(j) for j, b in enumerate(range(b0, n_calls, every))] if cand else []
        forced.append({f: deltas[(j * D + s) % len(deltas)][1] for j, f in enumerate(fixed)})
        if not fixed:
            pos = list(range((s * shift) % (P // 8), N, P))
        else:
            pos = list(range(fixed[0] % P, fixed[0], P))
            for fa, fb in zip(fixed, fixed[1:]):
                pos += list(range(fa, fb - lo + 1, P))
            pos += list(range(fixed[-1], N, P))
        out.append(np.array(pos, np.int64))
        assert np.all(np.diff(out[-1]) >= lo) and out[-1][0] >= 0 and out[-1][-1] < N
    return out, forced


def probe_input(n_calls, C, S, stages, every=1, shift=77, pos=None):
    """complex64 [S, n_calls * C], zero but for isolated samples from AMPS, and the positions (probe_positions unless given).  The amplitudes walk through
    AMPS; an impulse that designs a boundary takes the one of the same size and sign in the part its design names."""
    pos, forced = (pos, [{}] * len(pos)) if pos is not None else probe_positions(n_calls, C, S, stages, every, shift)
    x = np.zeros((S, n_calls * C), np.complex64)
    for s, p in enumerate(pos):
        k = np.arange(len(p))
        i = (k + k // len(AMPS) + 3 * s) % len(AMPS)              # (k // 8: so that neither part keeps to half of the residues modulo 8)
        for g, comp in forced[s].items():
            w = int(np.searchsorted(p, g))
            i[w] = i[w] % 4 + 4 * comp
        x[s, p] = AMPS[i]
    return x, pos


# ---- the float64 model -------------------------------------------------------------------------------------------------------------------------------
def _parts(x):
    return np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2).astype(np.float64)


def _terms(nz, D, T, out_n):
    """(output, tap, buffer index) of every product whose input is flagged in nz (buffer coordinates: T - 1 history entries in front)."""
    idx = np.flatnonzero(nz)
    o, t, i = [], [], []
    for j in range((T - 1) // D + 1):
        oo = idx // D - j
        tt = idx - oo * D
        ok = (oo >= 0) & (oo < out_n) & (tt < T)
        o.append(oo[ok]); t.append(tt[ok]); i.append(idx[ok])
    return np.concatenate(o), np.concatenate(t), np.concatenate(i)


def _pow2(v):
    v = v[v != 0]
    return bool(np.all(np.abs(np.frexp(v)[0]) == 0.5))


class Fir:
    """One FIR of the chain in float64 with its bound: D = 1 and alias = False for the low-pass, the oracle's decimator otherwise."""

    def __init__(self, taps, D=1, alias=True, bounds=True):
        self.k, self.D, self.alias, self.bounds = np.asarray(taps, np.float32).astype(np.float64), int(D), alias, bounds
        self.T = len(self.k)
        self.hx, self.he = np.zeros((self.T - 1, 2)), np.zeros((self.T - 1, 2))

    def __call__(self, x, e):
        n, T, D = len(x), self.T, self.D
        assert n >= T - 1, "push shorter than the stage's history (undefined in the reference)"
        out_n = n // D
        bx = np.concatenate([self.hx, x])
        be = np.concatenate([self.he, e]) if self.bounds else None
        if not self.bounds:                              # dense input, values only (the rms comparison of the arithmetic modes)
            y = np.stack([np.convolve(bx[:, c], self.k[::-1], "valid")[:out_n * D:D] for c in (0, 1)], axis=1)
            cx = x.copy()
            if self.alias:
                cx[:out_n] = y
            self.hx = cx[n - (T - 1):]
            return y, np.zeros_like(y), None
        exact = _pow2(bx) and not be.any()               # every product exact: one rounding less on a term's path
        y, ey, mm = np.zeros((out_n, 2)), np.zeros((out_n, 2)), np.zeros((out_n, 2), np.int64)
        ak = np.abs(self.k)
        for c in (0, 1):
            nz = (bx[:, c] != 0) | (be[:, c] != 0)
            if np.count_nonzero(nz) * ((T - 1) // D + 1) > 400000:       # dense input: whole correlations, every D-th kept
                cv = lambda v, w: np.convolve(v, w[::-1], "valid")[:out_n * D:D]
                A, E = cv(np.abs(bx[:, c]) + be[:, c], ak), cv(be[:, c], ak)
                m = np.rint(cv(nz.astype(np.float64), np.ones(T))).astype(np.int64)
                y[:, c], mm[:, c], ey[:, c] = cv(bx[:, c], self.k), m, gamma(m - 1 if exact else m) * A + E
                continue
            o, t, i = _terms(nz, D, T, out_n)
            y[:, c] = np.bincount(o, self.k[t] * bx[i, c], out_n)
            A = np.bincount(o, ak[t] * (np.abs(bx[i, c]) + be[i, c]), out_n)
            E = np.bincount(o, ak[t] * be[i, c], out_n)
            m = np.bincount(o, minlength=out_n)
            mm[:, c] = m
            ey[:, c] = gamma(m - 1 if exact else m) * A + E
        cx, ce = x.copy(), e.copy()
        if self.alias:                                   # Decimator.h:140-143: the outputs alias the input's head before the history is taken
            cx[:out_n], ce[:out_n] = y, ey
        self.hx, self.he = cx[n - (T - 1):], ce[n - (T - 1):]
        return y, ey, mm


def model(pushes, stages, lowpass_taps=None):
    """pushes: [n_calls, C] complex64 of ONE stream (for a front-tuned stream: hd_host_tune_rotate's output).  Per call a dict: y, e (float64 [n, 2]: real
    and imaginary part) and m of `decimated`, and -- where lowpass_taps is given and the call filters anything -- fy, fe of `filtered` (None otherwise), with f0: the
    decimated output (counted from the stream's start) that the call's first filtered output belongs to."""
    F = total_ratio(stages)
    firs = [Fir(k, r) for r, k in stages]
    lp = Fir(lowpass_taps, 1, alias=False) if lowpass_taps is not None else None
    qy, qe = np.zeros((0, 2)), np.zeros((0, 2))
    out, filtered = [], 0
    for x in pushes:
        assert len(x) % F == 0
        y, e, m = _parts(x), np.zeros((len(x), 2)), None
        for f in firs:
            y, e, m = f(y, e)
        r = dict(y=y, e=e, m=m, fy=None, fe=None, f0=filtered, lp_ntaps=lp.T if lp is not None else 0)
        if lp is not None:
            qy, qe = np.concatenate([qy, y]), np.concatenate([qe, e])
            if len(qy) >= LP_BATCH:
                n = len(qy) - len(qy) % LP_BATCH
                assert lp.T <= n + 1
                r["fy"], r["fe"], _ = lp(qy[:n], qe[:n])
                qy, qe = qy[n:], qe[n:]
                filtered += n
        out.append(r)
    return out


def model_values(pushes, stages):
    """`decimated` of every call in float64, without bounds (any input)."""
    firs = [Fir(k, r, bounds=False) for r, k in stages]
    out = []
    for x in pushes:
        y = _parts(x)
        for f in firs:
            y = f(y, None)[0]
        out.append(y)
    return out


def rms_to(got, y):
    return float(np.sqrt(np.mean((_parts(got) - y) ** 2)))


def worst(got, y, e):
    """(excess, flat index into [n, 2]) of the sample furthest out: |got - y| / e where e > 0; inf where e == 0 and got != y."""
    g = _parts(got)
    if g.shape != y.shape:
        return np.inf, -1
    d = np.abs(g - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e > 0, d / np.where(e > 0, e, 1.0), np.where(d == 0, 0.0, np.inf))
    if not r.size:
        return 0.0, -1
    i = int(np.argmax(r))
    return float(r.flat[i]), i


def excess(got, y, e):
    return worst(got, y, e)[0]


# ---- coverage: which tap indices the impulses exercise, and where ---------------------------------------------------------------------------------------
def stage1_hits(pos, R1, T1):
    """Every (impulse g, first-stage output o, tap t) with the impulse inside the output's window: t = g - o R1 + T1 - 1."""
    g = np.repeat(pos, (T1 - 1) // R1 + 1)
    o = -(-g // R1) + np.tile(np.arange((T1 - 1) // R1 + 1), len(pos))
    t = g - o * R1 + T1 - 1
    ok = t >= 0
    return g[ok], o[ok], t[ok]


def stage2_hits(pos, stages):
    """Every (impulse g, first-stage output o1, second-stage output o2, tap t2): t2 = o1 - o2 R2 + T2 - 1."""
    (R1, k1), (R2, k2) = stages
    g, o1, _ = stage1_hits(pos, R1, len(k1))
    T2, J = len(k2), (len(k2) - 1) // R2 + 1
    g, o1 = np.repeat(g, J), np.repeat(o1, J)
    o2 = -(-o1 // R2) + np.tile(np.arange(J), len(o1) // J)
    t2 = o1 - o2 * R2 + T2 - 1
    ok = t2 >= 0
    return g[ok], o1[ok], o2[ok], t2[ok]


def coverage(pos_per_stream, stages, C, n_calls, tiles=None, first_call=0):
    """Sets of tap indices exercised over a case: anywhere, through the history carry (impulse in push k, output in push k + 1) -- for both stages --, and,
    given the tiles of one push's schedule (rows of ring_schedule_main: k row0 out0 out_n chained last first_of_run), among the wrapped rows of
    a chained tile, in the first tile of a run and in the closing tile (the stream's last).  first_call: the first call that takes the case's route
    (first_worker_call): the carry counts only impulses in pushes from that one on, the tile positions only outputs of calls from that one on -- what
    call 0 computes on another route says nothing about this one."""
    R1, T1 = stages[0][0], len(stages[0][1])
    F = total_ratio(stages)
    rows = C // R1
    cov = dict(res1=set(), resF=set(), taps1=set(), carry1=set(), taps2=set(), carry2=set(), wrapped=set(), first=set(), closing=set())
    for pos in pos_per_stream:
        cov["res1"] |= set((pos % R1).tolist()); cov["resF"] |= set((pos % F).tolist())
        g, o, t = stage1_hits(pos, R1, T1)
        keep = o < n_calls * rows
        g, o, t = g[keep], o[keep], t[keep]
        cov["taps1"] |= set(t.tolist())
        cov["carry1"] |= set(t[(g // C < (o * R1) // C) & (g // C >= first_call)].tolist())
        if tiles is not None:
            row = o % rows
            for (k, row0, out0, out_n, chained, last, first) in tiles:
                inside = (row >= out0) & (row < out0 + out_n) & ((o * R1) // C >= first_call)
                if chained:
                    cov["wrapped"] |= set(t[inside & (row < out0 + tiles[0][2] - tiles[0][1])].tolist())
                if first:
                    cov["first"] |= set(t[inside].tolist())
                if last:
                    cov["closing"] |= set(t[inside].tolist())
        if len(stages) == 2:
            g, o1, o2, t2 = stage2_hits(pos, stages)
            keep = o2 < n_calls * C // F
            g, o1, o2, t2 = g[keep], o1[keep], o2[keep], t2[keep]
            cov["taps2"] |= set(t2.tolist())
            cov["carry2"] |= set(t2[(g // C < (o2 * F) // C) & ((o1 * R1) // C < (o2 * F) // C) & (g // C >= first_call)].tolist())
    return cov


def explain(o, k, s, pos, stages, C, tiles=None):
    """What a failure message needs about decimated output o of call k, stream s: the impulses inside its windows with their first- and second-stage tap
    indices, whether the window spans the push boundary, and the first-stage rows' places in the tile schedule."""
    R1, T1 = stages[0][0], len(stages[0][1])
    F = total_ratio(stages)
    O = k * (C // F) + o
    lines = []
    if len(stages) == 2:
        g, o1, o2, t2 = stage2_hits(pos, stages)
        sel = o2 == O
        for gg, oo1, tt2 in zip(g[sel], o1[sel], t2[sel]):
            lines.append(dict(impulse_at=int(gg), impulse_push=int(gg // C), stage1_output=int(oo1), stage1_tap=int(gg - oo1 * R1 + T1 - 1), stage2_tap=int(tt2),
                              stage1_row_in_push=int(oo1 % (C // R1)) if oo1 * R1 // C == k else ("previous push", int(oo1 % (C // R1))),
                              spans_push_boundary=bool(gg // C < k)))
    else:
        g, o1, t = stage1_hits(pos, R1, T1)
        sel = o1 == O
        for gg, tt in zip(g[sel], t[sel]):
            lines.append(dict(impulse_at=int(gg), impulse_push=int(gg // C), stage1_tap=int(tt), stage1_row_in_push=int(O % (C // R1)), spans_push_boundary=bool(gg // C < k)))
    if tiles is not None:
        for ln in lines:
            r = ln["stage1_row_in_push"]
            if isinstance(r, int):
                ln["tiles"] = [dict(tile=t[0], lane=r - t[1], chained=bool(t[4]), first_of_run=bool(t[6]), last=bool(t[5])) for t in tiles if t[2] <= r < t[2] + t[3]]
    return dict(stream=s, call=k, output=o, terms=lines)


def explain_filtered(o, k, s, f0, lp_ntaps, pos, stages, C, tiles=None):
    """The same for filtered output o of call k (the f0 + o-th of the stream): every impulse whose decimated response lies inside the low-pass's window,
    with the low-pass taps that response meets and, through explain(), the decimator taps, tile positions and push boundary of the response's samples."""
    R1, T1 = stages[0][0], len(stages[0][1])
    F = total_ratio(stages)
    Of = f0 + o
    if len(stages) == 2:
        g, _, o2, _ = stage2_hits(pos, stages)
    else:
        g, o2, _ = stage1_hits(pos, R1, T1)
    sel = (o2 <= Of) & (o2 > Of - lp_ntaps)
    lines = []
    for gg in np.unique(g[sel]):
        oo = o2[sel & (g == gg)]
        big = int(oo[len(oo) // 2])                                  # a sample from the middle of the response, explained down to the decimators' taps
        lines.append(dict(impulse_at=int(gg), impulse_push=int(gg // C), spans_push_boundary=bool(gg // C < k),
                          decimated_outputs=(int(oo.min()), int(oo.max())), lowpass_taps=(int(oo.min() - Of + lp_ntaps - 1), int(oo.max() - Of + lp_ntaps - 1)),
                          middle_sample=explain(big % (C // F), big // (C // F), s, pos, stages, C, tiles)))
    return dict(stream=s, call=k, filtered_output=o, decimated_output_of_stream=int(Of), terms=lines)


def check(got, res, what, k, s, pos, stages, C, tiles=None, fy=False):
    """Assert excess <= 1 for one read-out; the message names tap indices, stream, tile position and push boundary with got, y, e."""
    y, e = (res["fy"], res["fe"]) if fy else (res["y"], res["e"])
    ex, i = worst(got, y, e)
    if ex <= 1.0:
        return ex
    o, c = divmod(i, 2) if i >= 0 else (-1, 0)
    info = dict(what=what, excess=ex, component="re im".split()[c], shape_got=np.shape(got), shape_model=y.shape)
    if i >= 0:
        info.update(got=float(_parts(got)[o, c]), y=float(y[o, c]), e=float(e[o, c]))
        info.update(explain(o, k, s, pos, stages, C, tiles) if not fy else explain_filtered(o, k, s, res["f0"], res["lp_ntaps"], pos, stages, C, tiles))
    raise AssertionError(info)


# ---- a float32 emulation of the chain, for mutants ----------------------------------------------------------------------------------------------------
class Terms:
    """The non-zero products of one FIR call, from the pattern of its input alone (nz: bool [T - 1 + n, 2], the history in front): per output in tap
    order, grouped by their rank within the output (within each of the two chains for 'fma2') so that a run is one vector step per rank."""

    def __init__(self, nz, D, T, out_n):
        self.out_n, self.c = out_n, []
        for c in (0, 1):
            o, t, i = _terms(nz[:, c], D, T, out_n)
            order = np.lexsort((t, o))
            o, t, i = o[order], t[order], i[order]
            groups = {}
            for mode, sels in (("seq", [np.ones(len(o), bool)]), ("fma2", [t % 2 == 0, t % 2 == 1])):
                groups[mode] = []
                for sel in sels:
                    w = np.flatnonzero(sel)
                    oo = o[w]
                    start = np.flatnonzero(np.r_[True, oo[1:] != oo[:-1]]) if len(oo) else np.zeros(0, np.int64)
                    rank = np.arange(len(oo)) - np.repeat(start, np.diff(np.r_[start, len(oo)]))
                    groups[mode].append([w[rank == r] for r in range(int(rank.max()) + 1)] if len(oo) else [])
            self.c.append((o, t, i, groups))

    def touched(self):
        """bool [out_n, 2]: outputs with at least one product."""
        return np.stack([np.bincount(o, minlength=self.out_n) > 0 for o, _, _, _ in self.c], axis=1)

    def run(self, b, taps, mode):
        """mode 'seq': the oracle's loop (product and sum rounded separately, taps ascending); 'fma2': two chains (even and odd taps) of fused
        multiply-adds -- one rounding per a + x k, evaluated in float64 and rounded -- added at the end.  Zero inputs are skipped: their products are
        exact zeros."""
        y = np.zeros((self.out_n, 2), np.float32)
        for c, (o, t, i, groups) in enumerate(self.c):
            kk, xx = taps[t], b[i, c]
            accs = []
            for chain in groups[mode]:
                acc = np.zeros(self.out_n, np.float32)
                for w in chain:
                    if mode == "seq":
                        acc[o[w]] = acc[o[w]] + xx[w] * kk[w]
                    else:
                        acc[o[w]] = (acc[o[w]].astype(np.float64) + xx[w].astype(np.float64) * kk[w].astype(np.float64)).astype(np.float32)
                accs.append(acc)
            y[:, c] = accs[0] if mode == "seq" else accs[0] + accs[1]
        return y


class MutantBench:
    """One stream's FIRST push through the chain (zero history), with the term structure kept, so that a mutated table costs a few vector steps."""

    def __init__(self, x, stages, lowpass_taps=None):
        self.tables = [np.asarray(k, np.float32) for _, k in stages] + ([np.asarray(lowpass_taps, np.float32)] if lowpass_taps is not None else [])
        self.D = [r for r, _ in stages] + ([1] if lowpass_taps is not None else [])
        self.n_dec = len(stages)
        self.x = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
        self.terms, nz, n = [], self.x != 0, len(self.x)
        for j, (k, D) in enumerate(zip(self.tables, self.D)):
            if j == self.n_dec:
                n -= n % LP_BATCH
                nz = nz[:n]
            T = len(k)
            self.terms.append(Terms(np.concatenate([np.zeros((T - 1, 2), bool), nz]), D, T, n // D))
            nz, n = self.terms[-1].touched(), n // D

    def run(self, tables=None, mode="seq", start=0, inputs=None):
        """Outputs of every FIR, float32 [n, 2] each; `inputs`: an earlier run's list, reused in front of stage `start`."""
        tables = tables or self.tables
        outs = list(inputs[:start]) if inputs else []
        y = self.x if start == 0 else outs[start - 1]
        for j in range(start, len(tables)):
            if j == self.n_dec:
                y = y[:len(y) - len(y) % LP_BATCH]
            y = self.terms[j].run(np.concatenate([np.zeros((len(tables[j]) - 1, 2), np.float32), y]), tables[j], mode)
            outs.append(y)
        return outs

    def kills(self, j, y, e, out=-1):
        """Every mutant of table j: its excess over the bound (y, e) at FIR output `out` of the chain.  Returns {mutant: excess}."""
        base = self.run()
        res = {}
        for name, m in mutants(self.tables[j]):
            t = list(self.tables)
            t[j] = m
            got = self.run(t, start=j, inputs=base)[out]
            res[name] = excess(np.ascontiguousarray(got).view(np.complex64).reshape(-1), y, e)
        return res


def mutants(taps):
    """(name, mutated table) one at a time: every tap x (1 + 2^-10), every tap zeroed, adjacent taps swapped where they differ."""
    taps = np.asarray(taps, np.float32)
    for t in range(len(taps)):
        m = taps.copy(); m[t] = np.float32(m[t] * np.float32(1 + 2.0 ** -10)); yield ("scaled", t), m
        m = taps.copy(); m[t] = 0; yield ("zeroed", t), m
        if t + 1 < len(taps) and taps[t] != taps[t + 1]:
            m = taps.copy(); m[t], m[t + 1] = taps[t + 1], taps[t]; yield ("swapped", t), m


def schedule_tiles(exe, rows, hr, run_len, chained):
    """One push's tile schedule from host/ring_schedule.hpp, printed by the stand-alone schedule program (tests/ring_schedule_main.cpp with arguments):
    rows of (k, row0, out0, out_n, chained, last, first_of_run)."""
    import subprocess
    r = subprocess.run([str(exe), str(rows), str(hr), str(run_len), str(int(chained))], capture_output=True, text=True, timeout=60, check=True)
    return [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("tile ")]


def build_schedule_program(out_dir):
    import shutil
    import subprocess
    from pathlib import Path
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        return None
    exe = Path(out_dir) / "ring_schedule_main"
    subprocess.run([cxx, "-std=c++17", "-O1", str(Path(__file__).resolve().parent / "ring_schedule_main.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    return exe


# ---- the cases: shared by tests/test_fir_probe.py (layout conditions, the oracle inside the bound) and tests/test_gpu_fast_taps.py (the kernels) ------------
# `every`: a stream designs every such push boundary (probe_positions) -- the smallest stride at which at most 1 % of a case's outputs see no impulse at all,
# found by running the model over the layouts; `n`: calls (at least calls_needed()).  ring = (run length, chained): the worker waves' schedule of the case.
def _case(factor, fs, S, C, every, n=None, **kw):
    st = tables(factor)
    return dict(factor=factor, fs=fs, S=S, C=C, every=every, n=max(n or 0, calls_needed(S, st, every)), **kw)


PLAN_FACTORS = ((2, 1), (4, 1), (8, 1), (16, 1), (32, 2), (64, 3), (128, 4), (256, 8))        # (factor, every)
STEP_CASES = tuple((C, n, what) for C, n in ((4096, 70), (6144, 46)) for what in ("short0", "short100", "plain"))
# The names are static, so that collecting the tests needs no oracle library; the table itself wants the oracle's tap tables and is built on first use.
CASE_NAMES = tuple([f"plan_{f}" for f, _ in PLAN_FACTORS] + ["tail_64", "direct_16"] + [f"step_{C}_{what}" for C, _, what in STEP_CASES]
                   + ["stage1_alone", "plan128_halo", "percu_16", "percu_256", "tuned_64", "tuned_16"])
DENSE_NAMES = tuple([f"plan_{f}" for f, _ in PLAN_FACTORS] + [f"step_{C}_{what}" for C, _, what in STEP_CASES])     # k_decimate and k_step_cu


def _build_cases():
    c = {}
    for f, every in PLAN_FACTORS:
        c[f"plan_{f}"] = _case(f, 10e6 if f >= 128 else 0.4e6, 2, 65536, every, n=4, ungated=True, dense=True, filtered=True, classic=True,
                               env=dict(HD_NO_CLAIM="1"))     # (k_decimate on every call: without it the per-CU first stage takes over from the second call on)
    c["tail_64"] = _case(64, 2.048e6, 3, 65536, 3, path=2, filtered=True)
    c["direct_16"] = _case(16, 2.5e6, 2, 65536, 1, lowpass_bw=3000.0, path=0, filtered=True)
    envs = dict(short0=dict(HD_RING_SHORT_PCT="0"), short100=dict(HD_RING_SHORT_PCT="100"), plain=dict(HD_RING_CHAIN="0"))
    for C, n, what in STEP_CASES:           # (n: the fewest calls tried at which each part alone exercises every tap among the wrapped rows)
        c[f"step_{C}_{what}"] = _case(64, 2.048e6, 64, C, (n - 1) // 3, n=n, pipeline=2, path=3, variant=1, env=envs[what], ring=(4, what == "short0"), dense=True)
    c["stage1_alone"] = _case(64, 2.048e6, 64, 6144, 15, n=46, pipeline=0, variant=1, env={}, ring=(4, True))
    c["plan128_halo"] = _case(128, 2.048e6, 64, 65536, 5, n=16, pipeline=2, path=3, variant=1, env=dict(HD_RING_SHORT_PCT="0"), ring=(4, True))
    c["percu_16"] = _case(16, 2.5e6, 8, 16384, 3, lowpass_bw=3000.0, device=True, first_call_classic=True)
    c["percu_256"] = _case(256, 10e6, 8, 16384, 9, n=200, device=True, first_call_classic=True)
    c["tuned_64"] = _case(64, 2.048e6, 4, 65536, 3, tune=[0.0, 123456.7, -400e3, 7.3], filtered=True, classic=True)
    c["tuned_16"] = _case(16, 2.5e6, 4, 8192, 3, tune=[0.0, 123456.7, -400e3, 7.3], filtered=True, classic=True)
    assert tuple(c) == CASE_NAMES and tuple(k for k in c if c[k].get("dense")) == DENSE_NAMES
    return c


_cases = {}


def cases():
    if not _cases:
        _cases.update(_build_cases())
    return _cases


def first_worker_call(c):
    """The first call of a case that takes the route the case is about: a stream's first call restarts its history on the classic grid (step variant 0)
    where the case runs the worker waves or the per-CU first stage; everywhere else call 0 already is the route."""
    return 1 if ("variant" in c or c.get("first_call_classic")) else 0


def layout_key(c):
    return (c["factor"], c["fs"], c["S"], c["C"], c["every"], c["n"], tuple(c.get("tune", ())), c.get("lowpass_bw"), bool(c.get("filtered")))


def case_input(c):
    """(x [S, n C] complex64, positions per stream, stages) of a case."""
    st = tables(c["factor"])
    x, pos = probe_input(c["n"], c["C"], c["S"], st, c["every"])
    return x, pos, st


def halo_rows(stages):
    R1, T1 = stages[0][0], len(stages[0][1])
    return (T1 - 1 + R1 - 1) // R1
