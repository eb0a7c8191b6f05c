"""Inputs that drive the discriminator (kernels/exact_math.h: discriminate, exact_atan2f_plain, exact_atan2f) over its whole domain, and a classifier that
says, from the oracle's low-pass output, which part of that domain every product cur * conj(prev) falls in.

Why a builder: RTTY plus noise behind the default low-pass keeps every product in the right half-plane with |im / re| < 7/16 -- one of the twenty cells
(4 quadrants x 5 reduction intervals of atanf) of the straight-line function, and none of the special cases of the general one but exact zeros.

How the low-pass output is controlled.  lowpass_trans = 0.8 gives a FIVE-tap low-pass (T = 5: about 3.5e-5, 0.151, 0.697, 0.151, 3.5e-5), so the filtered
samples follow the decimated ones closely.  At decimation = 1 the input IS the low-pass's input.  Behind two decimation stages the input is zero-stuffed,
x[D * m + T0] = D * d[m]: the decimated samples are `d` through a real FIR.  That FIR is NOT short: measured on the oracle, an impulse in `d` reaches 37
decimated samples (38 for T0 = 0 and T0 = D - 1) at /64 and at /16 alike -- the second stage's 69 taps at two inputs per output, no empty polyphase
branch.  A stretch of `d` therefore stands alone only behind SPREAD + T + 1 zeros, and that is what separates the blocks of a two-stage stream (`gap`).

Streams (each case of tests/test_gpu_discriminator_domain.py carries all four, PATTERNS):
  clean    ordinary products only: random phases with log-uniform magnitudes, then dense angle sweeps across the edges of the reduction intervals in every
           quadrant.  Every wave of the device takes exact_atan2f_plain.
  clean2   the same with another seed.
  planted  the same ordinary material in pieces, a run of zeros behind each piece (exactly zero low-pass outputs at least every 192 outputs, the bound the CPU
           test checks; a wave spans 256 outputs or more), so that every wave takes exact_atan2f; then the special blocks whose discriminator outputs
           are all finite (`special_blocks`).  Bits and backlog are compared on it.
  wild     planted, and the blocks that put a NaN into the discriminator's output: a hold of (2^100, 2^100) (both products infinite, im = Inf - Inf), one NaN
           sample, one Inf sample.

Classes of the general function.  `X_ONE` (re == 1.0f exactly, im != 0: atan2f's `x == 1` shortcut) is reached at decimation = 1 only where `unit_hold` finds
an input whose five-tap sum rounds to exactly 1.0f; it is reported, never required -- behind two stages no input value is known to give 1.0f, and the
required classes stay as they are.  Filtered parts are never -0 (a sum that starts at +0.0f cannot end at -0), so im = -0 with re > 0 cannot come from
pure-real or pure-imaginary stretches: it comes from two products that both underflow from below (`underflow_block`).

The Python copies of atan2_plain_args / atan2_plain_quotient below only say which device path a product takes; no expected VALUE is computed here."""
import numpy as np

T = 5                      # low-pass taps with LOWPASS_TRANS
LOWPASS_TRANS = 0.8
SPREAD = 37                # decimated samples one `d` reaches behind two stages with T0 = 1 (measured on the oracle; module docstring)
T0 = 1                     # where in its D input samples a stuffed sample stands
EDGES = (7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16)
INTERVAL_BITS = (0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000)
PATTERNS = ("clean", "planted", "wild", "clean2")

SPECIALS = ("both_zero", "im+0_re>0", "im-0_re>0", "im+0_re<0", "im-0_re<0", "re0_im>0", "re0_im<0", "re_inf", "im_inf", "both_inf", "nan", "k>60",
            "k<-60_re<0", "k<-60_re>0", "quotient_tiny", "quotient_huge", "denormal_product", "denormal_quotient")
REQUIRED_TWO_STAGE = ("both_zero", "im+0_re>0", "im-0_re>0", "im+0_re<0", "im-0_re<0", "re0_im>0", "re0_im<0", "nan", "k>60", "k<-60_re<0")
OPTIONAL = ("x_one",)


# ---- classifier
def products(filtered, prev):
    """re, im, |im / re| of every discriminator input of a call, in float32 with discriminate's operation order; prev: the sample in front of the call."""
    f = np.ascontiguousarray(filtered, np.complex64)
    p = np.concatenate([np.array([prev], np.complex64), f[:-1]])
    a, b, c, d = f.real.copy(), f.imag.copy(), p.real.copy(), -p.imag
    with np.errstate(all="ignore"):
        re = (a * c) - (b * d)
        im = (a * d) + (b * c)
        t = np.abs(im / re)
    assert re.dtype == np.float32 and t.dtype == np.float32
    return re, im, t


def classify(filtered, prev):
    """dict: 'plain' (bool per product: the straight-line function's domain), 'cell' (quadrant * 5 + interval for plain products, -1 otherwise), and one bool
    array per name of SPECIALS + OPTIONAL (a product may carry several)."""
    re, im, t = products(filtered, prev)
    hx, hy, ht = re.view(np.uint32).astype(np.int64), im.view(np.uint32).astype(np.int64), t.view(np.uint32).astype(np.int64)
    sx, sy = hx >> 31, hy >> 31
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    k = (iy - ix) >> 23
    INF = 0x7f800000
    # atan2_plain_args and atan2_plain_quotient
    args = (ix != 0) & (iy != 0) & (ix < INF) & (iy < INF) & (hx != 0x3f800000) & (k <= 60) & (k >= -60)
    quot = (ht >= 0x31000000) & (ht < 0x4c000000)
    plain = args & quot
    interval = sum((ht >= e).astype(np.int64) for e in INTERVAL_BITS)
    out = {"plain": plain, "cell": np.where(plain, (2 * sx + sy) * 5 + interval, -1), "re": re, "im": im, "t": t}
    nan = (ix > INF) | (iy > INF)
    fin = ~nan
    ord_ = fin & (ix != 0) & (iy != 0) & (ix < INF) & (iy < INF)
    out["nan"] = nan
    out["both_zero"] = fin & (ix == 0) & (iy == 0)
    for m, name in enumerate(("im+0_re>0", "im-0_re>0", "im+0_re<0", "im-0_re<0")):
        out[name] = fin & (iy == 0) & (ix != 0) & ((2 * sx + sy) == m)
    out["re0_im>0"] = fin & (ix == 0) & (iy != 0) & (sy == 0)
    out["re0_im<0"] = fin & (ix == 0) & (iy != 0) & (sy == 1)
    out["both_inf"] = (ix == INF) & (iy == INF)
    out["re_inf"] = (ix == INF) & (iy < INF) & (iy != 0)
    out["im_inf"] = (iy == INF) & (ix < INF) & (ix != 0)
    out["k>60"] = ord_ & (k > 60)
    out["k<-60_re<0"] = ord_ & (k < -60) & (sx == 1)
    out["k<-60_re>0"] = ord_ & (k < -60) & (sx == 0)
    out["quotient_tiny"] = args & (ht < 0x31000000)
    out["quotient_huge"] = args & (ht >= 0x4c000000)
    den = lambda i: (i != 0) & (i < 0x00800000)
    out["denormal_product"] = fin & (den(ix) | den(iy))
    out["denormal_quotient"] = ord_ & den(ht)
    out["x_one"] = fin & (hx == 0x3f800000) & (iy != 0)
    return out


def longest_plain_run(plain):
    best = run = 0
    for p in plain:
        run = run + 1 if p else 0
        best = max(best, run)
    return best


# ---- building blocks (all in the decimated domain: `d`)
def random_phase(n, span, rng, walk):
    """Uniform phases; magnitudes 2^e, e a random walk over [-span, span] with steps up to `walk`: log-uniform in the long run, but neighbours stay within the
    24 bits of a float of each other.  With independent magnitudes the low-pass output around a large sample is that sample times one tap after the other,
    and the product of two such outputs has im = 0 exactly (1182 of 16384 products at decimation = 1 with +-2^40): no ordinary product."""
    e = np.empty(n)
    x = rng.uniform(-span, span)
    for i, s in enumerate(rng.uniform(-walk, walk, n)):
        x += s
        if abs(x) > span:
            x = np.sign(x) * (2 * span - abs(x))
        e[i] = x
    return (2.0 ** e * np.exp(1j * rng.uniform(0, 2 * np.pi, n))).astype(np.complex64)


def sweeps(npts, lead):
    """Unit-magnitude rotations whose step walks, 1e-7 per sample, across atan(edge) in each quadrant -- a steady rotation passes any real FIR as the same
    rotation, so the products' |im / re| straddle every interval edge densely.  `lead` samples at the first step let a long FIR settle."""
    steps = []
    for e in EDGES:
        th = np.arctan(e)
        for centre in (th, -th, np.pi - th, th - np.pi):
            steps.append(np.full(lead, centre - (npts // 2) * 1e-7))
            steps.append(centre + (np.arange(npts) - npts // 2) * 1e-7)
    ph = np.cumsum(np.concatenate(steps))
    return np.exp(1j * ph).astype(np.complex64)


def ordinary(seed, n_random, span, walk, npts, lead):
    rng = np.random.default_rng(seed)
    return np.concatenate([random_phase(n_random, span, rng, walk), sweeps(npts, lead)])


def unit_hold():
    """An input value v whose five-tap sum (float32, the FIR's order) is exactly 1.0f, or None: what `x == 1` needs at decimation = 1.  The taps are those of
    the 1500 Hz / 32 kHz design as the oracle computes them; the CPU test checks the class on the oracle, not this arithmetic."""
    from oracle import pyoracle
    o = pyoracle.Decoder("oracle", factor=1, lowpass_trans=LOWPASS_TRANS, ungated=True, with_fft=False)
    o(np.ones(256, np.complex64), 32000.0)
    taps = o.array("fir_taps")
    v = np.float32(1.0) / np.float32(taps.astype(np.float64).sum())
    for _ in range(64):
        acc = np.float32(0)
        for k in taps:
            acc = np.float32(acc + np.float32(v * k))
        if acc == np.float32(1.0):
            return v
        v = np.nextafter(v, np.float32(2.0 if acc < 1 else 0.0), dtype=np.float32)
    return None


def special_blocks(gap, hold, impulse_gap, big, seed, wild, one=None, im_inf=True):
    """The special material, every block behind `gap` zeros.  hold: samples a value is held for the low-pass output to reach it (T + 1 at decimation = 1);
    impulse_gap: distance of two impulses whose responses are T - 1 zeros apart."""
    rng = np.random.default_rng(seed)
    z = np.zeros(gap, np.complex64)
    H = lambda re, im: np.full(hold, complex(re, im), np.complex64)
    blocks = []
    # pure-real and pure-imaginary stretches with sign changes: im = +-0 with re on either side of zero
    r = rng.standard_normal(48).astype(np.float32)
    blocks += [r.astype(np.complex64), (1j * rng.standard_normal(48)).astype(np.complex64)]
    # impulses whose low-pass responses stand T - 1 zeros apart: re = 0 with im != 0, either sign
    for v1, v2 in ((1, 1j), (1, -1j), (1j, 1), (-1j, 1)):
        b = np.zeros(impulse_gap + 1, np.complex64)
        b[0], b[impulse_gap] = v1, v2
        blocks.append(b)
    # re overflows, im finite (between the holds); parts swapped: the same through the other product
    blocks.append(np.concatenate([H(2.0 ** 100, 2.0 ** -20), H(2.0 ** 100, -2.0 ** -20), H(2.0 ** 100, 2.0 ** -20)]))
    blocks.append(np.concatenate([H(2.0 ** -20, 2.0 ** 100), H(-2.0 ** -20, 2.0 ** 100), H(2.0 ** -20, 2.0 ** 100)]))
    # im overflows, re finite: two impulses again (the low-pass's end taps, 3.5e-5 each: re = a*c = 2^-20, im = b*c = 2^160), either sign
    # (decimation = 1 only: behind two stages the far ends of the two responses, 2^110 times taps of 1e-9, meet in one low-pass output: Inf - Inf)
    for sgn in (1, -1) if im_inf else ():
        b = np.zeros(impulse_gap + 1, np.complex64)
        b[0], b[impulse_gap] = 2.0 ** 110, complex(2.0 ** -100, sgn * 2.0 ** 80)
        blocks.append(b)
    # denormal products; a denormal quotient (im = b * c = 2^-149 over re = 2^-20)
    blocks.append(np.concatenate([H(2.0 ** -70, 2.0 ** -72), H(2.0 ** -70, -2.0 ** -72), H(-2.0 ** -71, 2.0 ** -70)]))
    blocks.append(np.concatenate([H(2.0 ** -10, 0.0), H(2.0 ** -10, 2.0 ** -139), H(2.0 ** -10, 0.0)]))
    blocks.append(underflow_block(hold))
    # k > 60: a real run of magnitude 1, then imaginary samples of `big` (2^80 at decimation = 1: the low-pass's 3.5e-5 end tap lets 2^65 in beside a real
    # part still 1; behind two stages the decimator's own end tap comes on top, so 2^110); the mirror; a quotient of 2^30 (beyond atanf's 2^25, k = 30);
    # k < -60 with re < 0 and with re > 0: a real run of 1, then (-+big, 1)
    blocks.append(np.concatenate([H(1, 0), H(0, big)]))
    blocks.append(np.concatenate([H(0, 1), H(big, 0)]))
    blocks.append(np.concatenate([H(1, 0), H(0, big * 2.0 ** -35)]))
    blocks.append(np.concatenate([H(1, 0), H(-big, 1)]))
    blocks.append(np.concatenate([H(1, 0), H(big, 1)]))
    if one is not None:                                              # re == 1.0f exactly beside an imaginary part that leaves 0
        blocks.append(np.concatenate([H(one, 0), H(one, 0.25), H(one, -3.0)]))
    if wild:
        blocks.append(np.concatenate([H(2.0 ** 100, 2.0 ** 100), H(-2.0 ** 100, 2.0 ** 100)]))
        blocks.append(np.concatenate([H(2.0 ** 100, 2.0 ** -30), H(2.0 ** -30, 2.0 ** 100), H(-2.0 ** 100, 2.0 ** -30)]))     # a quarter turn of a large hold
        for bad in (complex(np.nan, 0.5), complex(np.inf, -0.5)):
            b = random_phase(2 * hold + 1, 2, rng, 1)
            b[hold] = bad
            blocks.append(b)
    out = []
    for b in blocks:
        out += [z, b.astype(np.complex64)]
    return np.concatenate(out + [z])


def underflow_block(hold):
    """im = -0 beside re > 0: both products of im = a*d + b*c underflow from below (a, c > 0; the imaginary part goes from +2^-100 to -2^-100)."""
    H = lambda re, im: np.full(hold, complex(re, im), np.complex64)
    return np.concatenate([H(2.0 ** -60, 2.0 ** -100), H(2.0 ** -60, -2.0 ** -100), H(2.0 ** -60, 2.0 ** -100)])


def planted_pieces(material, piece, zeros):
    out = []
    for i in range(0, len(material), piece):
        out += [material[i:i + piece], np.zeros(zeros, np.complex64)]
    return np.concatenate(out)


# ---- the cases
# n: decimated samples per stream (a multiple of 256 and of push / factor); push: input samples per call
CASES = {
    "factor1": dict(factor=1, fs=32000.0, n=32768, push=16384, span=40, walk=6, big=2.0 ** 80, n_random=9000, npts=300, lead=8, piece=50, zeros=T + 1, gap=T + 1, hold=T + 1, impulse_gap=T),
    "d64": dict(factor=64, fs=2.048e6, n=8192, push=4096, span=20, walk=2, big=2.0 ** 110, n_random=1000, npts=64, lead=SPREAD + T, piece=110, zeros=SPREAD + T + 3, gap=SPREAD + T + 3,
                hold=SPREAD + T + 3, impulse_gap=SPREAD + T - 1),
    "d16": dict(factor=16, fs=0.512e6, n=8192, push=4096, span=20, walk=2, big=2.0 ** 110, n_random=1000, npts=64, lead=SPREAD + T, piece=110, zeros=SPREAD + T + 3, gap=SPREAD + T + 3,
                hold=SPREAD + T + 3, impulse_gap=SPREAD + T - 1),
}
_cache = {}


def decimated_domain(case, pattern):
    c = CASES[case]
    seed = 11 if pattern != "clean2" else 12
    mat = ordinary(seed, c["n_random"], c["span"], c["walk"], c["npts"], c["lead"])
    if pattern in ("clean", "clean2"):
        d = mat
        fill = random_phase(c["n"], c["span"], np.random.default_rng(seed + 100), c["walk"])
        d = np.concatenate([d, fill])[:c["n"]]
    else:
        one = unit_hold() if c["factor"] == 1 else None
        d = np.concatenate([planted_pieces(mat, c["piece"], c["zeros"]), special_blocks(c["gap"], c["hold"], c["impulse_gap"], c["big"], seed + 1, pattern == "wild", one, c["factor"] == 1)])
        assert len(d) <= c["n"], (case, pattern, len(d))
        fill = planted_pieces(random_phase(c["n"] // 2, c["span"], np.random.default_rng(seed + 100), c["walk"]), c["piece"], c["zeros"])
        d = np.concatenate([d, fill])[:c["n"]]
    return d.astype(np.complex64)


def stream(case, pattern):
    """The input of one stream: complex64 [n * factor]."""
    key = (case, pattern)
    if key not in _cache:
        c = CASES[case]
        d = decimated_domain(case, pattern)
        D = c["factor"]
        if D == 1:
            x = d
        else:
            x = np.zeros(len(d) * D, np.complex64)
            with np.errstate(invalid="ignore"):
                x[T0::D] = d * np.float32(D)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def oracle_run(case, pattern, taps_trans=LOWPASS_TRANS):
    """The oracle over the stream, call by call: a list of dicts (decimated, filtered, demod, bits, held, prev: the filtered sample in front of the call)."""
    key = (case, pattern, "oracle", taps_trans)
    if key in _cache:
        return _cache[key]
    from oracle import pyoracle
    c = CASES[case]
    o = pyoracle.Decoder("oracle", factor=c["factor"], baud=300, bits=8, stops=2, lowpass_trans=taps_trans, ungated=c["factor"] == 1, with_fft=False)
    x = stream(case, pattern)
    calls, prev = [], None
    for k in range(len(x) // c["push"]):
        o(x[k * c["push"]:(k + 1) * c["push"]], c["fs"])
        f = o.array("last_filtered")
        if prev is None and len(f):
            prev = f[0]
        calls.append(dict(decimated=o.array("last_decimated"), filtered=f, demod=o.array("last_demod"), bits=o.bits(), held=o.symex_held(), prev=prev,
                          ntaps=len(o.array("fir_taps"))))
        if len(f):
            prev = f[-1]
    _cache[key] = calls
    return calls


def census(case, pattern, taps_trans=LOWPASS_TRANS):
    """Classes of every product of the stream: (cells: 20 counts, specials: name -> count, longest run of plain products, demod NaN count)."""
    cells = np.zeros(20, np.int64)
    counts = {k: 0 for k in SPECIALS + OPTIONAL}
    plain_all = []
    bad = 0
    for call in oracle_run(case, pattern, taps_trans):
        if not len(call["filtered"]):
            continue
        cl = classify(call["filtered"], call["prev"])
        cells += np.bincount(cl["cell"][cl["cell"] >= 0], minlength=20)
        for k in counts:
            counts[k] += int(cl[k].sum())
        plain_all.append(cl["plain"])
        bad += int((~np.isfinite(call["demod"])).sum())
    plain = np.concatenate(plain_all)
    return cells, counts, longest_plain_run(plain), int((~plain).sum()), bad


# ---- flip search: RTTY streams with non-finite samples beside bit edges, and an integer-weight stream with interior first maxima
FLIP = dict(fs=2.048e6, factor=64, baud=300, bits=8, stops=2, push=65536, calls=44)
FLIP_STREAMS = ("plain", "nan_idle", "nan_edges", "inf_edges")


def _flip_base(seed):
    text = synth_sentence(seed) * 3                    # (the last sentence stays in the text stage until more text follows: two are delivered)
    from habdec_amd import synth
    n = FLIP["push"] * FLIP["calls"]
    x = synth.fsk_iq(synth.rtty_bits(text, FLIP["bits"], FLIP["stops"], 40, 10), FLIP["fs"], FLIP["baud"], sigma=0.05, seed=seed, n_samples=n)
    assert len(x) == n
    return x


def synth_sentence(seed):
    from habdec_amd import synth
    return synth.make_sentence(f"F{seed}", "1")


def flip_oracle(x, lookup=1, lowpass_bw=None):
    """The oracle over x call by call, with the flip points of every call: a second symbol extractor (the oracle's stage object, which exposes them) is fed the
    decoder's discriminator output exactly as the decoder feeds its own -- its bits must be the decoder's.  Returns (calls, decoder)."""
    from oracle import pyoracle
    o = pyoracle.Decoder("oracle", factor=FLIP["factor"], baud=FLIP["baud"], bits=FLIP["bits"], stops=FLIP["stops"], mathh_context=lookup, lowpass_bw=lowpass_bw,
                         with_fft=False)
    sx = pyoracle.Stages("oracle").symex(FLIP["fs"] / FLIP["factor"], FLIP["baud"])
    sx.abs_mode(lookup)
    calls, backlog = [], np.zeros(0, np.float32)
    for k in range(len(x) // FLIP["push"]):
        o(x[k * FLIP["push"]:(k + 1) * FLIP["push"]], FLIP["fs"])
        dm = o.array("last_demod")
        sx.push(dm)
        bits = sx.run()
        flips = sx.last_flips()
        assert np.array_equal(bits, o.bits()) and sx.held() == o.symex_held(), k
        before = np.concatenate([backlog, dm])
        backlog = before[int(flips[-1]):] if len(flips) else before
        assert len(backlog) == sx.held()
        calls.append(dict(demod=dm, decimated=o.array("last_decimated"), bits=bits, flips=flips, held=sx.held(), backlog=before, chars=o.text("chars_log"),
                          sentences=tuple(o.sentences())))
    return calls, o


def _windows(v, R):
    """Sums of v[i - R : i] (left) and v[i : i + R] (right) for R <= i <= len(v) - R, added in element order in float32 like SymbolExtractor.h:51-63."""
    w = np.lib.stride_tricks.sliding_window_view(np.ascontiguousarray(v, np.float32), R)
    with np.errstate(all="ignore"):
        s = np.cumsum(w, axis=1, dtype=np.float32)[:, -1]
    return s[:len(s) - R], s[R:]            # left[j], right[j] belong to i = R + j


def zones(call, R):
    """(lo, flip) of every flip point of a call: lo = the first position of the flip's edge zone, from the signs of the window averages."""
    v, out, off = call["backlog"], [], 0
    if not len(call["flips"]):
        return out
    left, right = _windows(v, R)
    sg = lambda a: (a > 0).astype(np.int8) - (a < 0).astype(np.int8)
    differ = sg(left) != sg(right)
    for f in call["flips"]:
        i = off + R
        while not differ[i - R]:
            i += 1
        out.append((i, int(f)))
        off = int(f)
    return out


def nonfinite_spans(demod_all):
    bad = np.nonzero(~np.isfinite(demod_all))[0]
    return (int(bad[0]), int(bad[-1])) if len(bad) else None


def flip_streams():
    """name -> input.  `plain` carries two sentences; the others are `plain` with non-finite samples:
      nan_idle   one NaN in the idle carrier in front of the text, more than 2 R from any edge;
      nan_edges  two NaN samples, placed (by measuring where the oracle's discriminator output turns NaN) so that one NaN stretch ENDS R / 2 before a bit edge
                 and the other BEGINS R / 2 behind one;
      inf_edges  the same two places with +Inf and -Inf in consecutive samples: the FIR sums, and with them the window sums, hold Inf - Inf."""
    if "flip_streams" in _cache:
        return _cache["flip_streams"]
    from oracle import pyoracle
    D, R = FLIP["factor"], int(round(FLIP["fs"] / FLIP["factor"] / FLIP["baud"])) // 4
    x = _flip_base(5)
    calls, _ = flip_oracle(x)
    dm = np.concatenate([c["demod"] for c in calls])
    # bit edges of the clean stream: sign changes of the R-sample moving average, first one past the idle lead-in
    avg = np.convolve(dm.astype(np.float64), np.ones(R) / R, "same")
    edges = np.nonzero(np.signbit(avg[1:]) != np.signbit(avg[:-1]))[0] + 1
    edges = edges[(edges > 2000) & (edges < len(dm) - 2000)]
    assert len(edges) > 40
    # where does a NaN at input sample p show up?  measured once, at p0; it moves by one output per D input samples
    p0 = 40 * D
    probe = x.copy(); probe[p0] = np.nan
    o = pyoracle.Decoder("oracle", factor=D, baud=FLIP["baud"], bits=FLIP["bits"], stops=FLIP["stops"], with_fft=False)
    o(probe[:FLIP["push"]], FLIP["fs"])
    first, last = nonfinite_spans(o.array("last_demod"))
    e1, e2 = int(edges[len(edges) // 3]), int(edges[2 * len(edges) // 3])
    p_end_before = p0 + D * ((e1 - R // 2) - last)            # the stretch ends R / 2 before e1
    p_begin_behind = p0 + D * ((e2 + R // 2) - first)         # the stretch begins R / 2 behind e2
    out = {"plain": x}
    idle = x.copy(); idle[p0 + 17] = np.nan
    out["nan_idle"] = idle
    ne = x.copy(); ne[p_end_before] = np.nan; ne[p_begin_behind] = np.nan
    out["nan_edges"] = ne
    ie = x.copy()
    for p in (p_end_before, p_begin_behind):
        ie[p], ie[p + 1] = np.inf, -np.inf
    out["inf_edges"] = ie
    for v in out.values():
        v.setflags(write=False)
    _cache["flip_streams"] = out
    _cache["flip_edges"] = (e1, e2, R, last - first + 1)
    return out


def flip_results(name):
    key = ("flip_results", name)
    if key not in _cache:
        _cache[key] = flip_oracle(flip_streams()[name])[0]
    return _cache[key]


# (the low-pass: hd "lowpass_bw" b designs sin(2 b n / fs) / (2 b n / fs), which cuts at b / pi -- 1.6 kHz for 5000, and two tones 5.1 kHz apart, the least whose
# averages differ by 1.0, do not pass that, whatever the carrier offset: measured on the oracle, every shift up to 4 kHz leaves all weights 0 and from 5.2 kHz
# on nothing decodes.  12000 cuts at 3.8 kHz and lets +-3.5 kHz through)
INT = dict(shift=7000.0, lowpass_bw=12000.0, sigma=0.02)


def integer_weight_stream():
    """lookup_mode = 0: the flip weight is (float)abs((int)(avg_r - avg_l)).  A 7 kHz shift puts the two tones 1.37 rad apart at 32 kS/s, so the weight is 0 at
    the rim of an edge zone and 1 on a plateau inside: the first maximum is an interior position, found among equal weights by index alone.  No NaN here:
    (int)NaN is undefined in the reference."""
    if "int_stream" not in _cache:
        from habdec_amd import synth
        n = FLIP["push"] * FLIP["calls"]
        x = synth.fsk_iq(synth.rtty_bits(synth_sentence(9) * 3, FLIP["bits"], FLIP["stops"], 40, 10), FLIP["fs"], FLIP["baud"], shift=INT["shift"], sigma=INT["sigma"], seed=9,
                         n_samples=n)
        x.setflags(write=False)
        _cache["int_stream"] = x
        _cache["int_results"] = flip_oracle(x, lookup=0, lowpass_bw=INT["lowpass_bw"])[0]
    return _cache["int_stream"], _cache["int_results"]
