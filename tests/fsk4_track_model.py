"""A numpy model of the 4FSK tone tracker, written from its definition (include/habdec_amd.h, "4FSK tone tracker") and not from the C++: what
hd_host_fsk4_comb_detect, hd_host_fsk4_track_* and the records of k_fsk4_comb are held to byte for byte.  Also the retune of the 4FSK modem
(hd_fsk4_retune) on top of tests/fsk4_model.py, which stays as it is, and the signals the tracker's tests share.

The detector is all here.  The spectrum is not part of the tracker's definition -- it is the tone search's -- so the model takes each segment's
|X|^2 from the tone search's restatement (one segment pushed into a fresh stream) and does the sums, the epochs and the decay itself, in float64."""
import math

import numpy as np

import fsk4_model as FM
import tones_model as TM

N = 4096
HOP = 2048
DEFAULTS = dict(epoch_segments=4, decay_q8=128, min_quality_q8=192, min_segments=4, deadband=8)


def floor_div(a, b):
    return a // b                                                    # Python's // is the floor


# ---- the detector

def comb_plan(fsd, baud, spacing_lo, spacing_hi, f_lo, f_hi):
    """Steps 4, 5 and 8 in front of the spectrum.  'unsupported' / 'invalid' as the header says, else the plan's integers."""
    if not (fsd > 0 and baud > 0 and spacing_lo > 0 and spacing_hi >= spacing_lo and f_hi > f_lo):
        return "invalid"
    if spacing_lo < 2.0 * baud:
        return "unsupported"
    b = fsd / N
    wd = np.rint(0.5 * baud / b)
    if not wd < N / 8:
        return "invalid"
    w = max(3, int(wd) | 1)
    h = w // 2
    b_lo, b_hi = max(0, N // 2 + math.ceil(f_lo / b)), min(N - 1, N // 2 + math.floor(f_hi / b))
    if b_lo > b_hi:
        return "invalid"
    if spacing_lo == spacing_hi:
        d_lo = d_hi = int(np.rint(4.0 * spacing_lo / b))
    else:
        d_lo, d_hi = math.ceil(4.0 * spacing_lo / b), math.floor(4.0 * spacing_hi / b)
    d_hi = min(d_hi, 4 * N)
    if d_lo < 4 or d_lo > d_hi or b_lo + 2 * h + ((3 * d_lo + 2) >> 2) > b_hi:
        return "invalid"
    while b_lo + 2 * h + ((3 * d_hi + 2) >> 2) > b_hi:
        d_hi -= 1
    return dict(w=w, d_lo=d_lo, d_hi=d_hi, b_lo=b_lo, b_hi=b_hi, known=int(spacing_lo == spacing_hi))


ZERO = dict(f0_q8=0, spacing_q8=0, c0=0, d=0, w=0, floor=0, score=0, quality_q8=0, valid=0, centroid_q8=[0, 0, 0, 0])


def comb_detect(acc, plan, min_quality_q8=192, segments_ok=True):
    """Steps 1 .. 9 on 4096 fftshifted sums: the record as a dict."""
    acc = np.asarray(acc, np.float64)
    assert acc.shape == (N,)
    if not np.all(np.isfinite(acc)) or not acc.max() > 0:
        return dict(ZERO)
    q = np.where(acc > 0, np.floor(acc / acc.max() * 524288.0), 0.0).astype(np.int64)
    floor = int(np.sort(q)[N // 2 - 1])
    ps = np.concatenate([[0], np.cumsum(q)])
    w, h = plan["w"], plan["w"] // 2
    B = np.zeros(N, np.int64)
    B[h:N - h] = ps[w:] - ps[:N - w + 1]                            # B[c] = ps[c + h + 1] - ps[c - h]
    best = None
    for d in range(plan["d_lo"], plan["d_hi"] + 1):
        o = [(t * d + 2) >> 2 for t in range(4)]
        first, last = plan["b_lo"] + h, plan["b_hi"] - h - o[3]
        sc = np.minimum(np.minimum(B[first:last + 1], B[first + o[1]:last + o[1] + 1]), np.minimum(B[first + o[2]:last + o[2] + 1], B[first + o[3]:last + o[3] + 1]))
        k = int(np.argmax(sc))                                       # the first of equals: the lowest c0
        if best is None or int(sc[k]) > best[0]:                     # strictly: the lowest d
            best = (int(sc[k]), d, first + k)
    score, d, c0 = best
    cen = []
    for t in range(4):
        c = c0 + ((t * d + 2) >> 2)
        cf = 256 * c
        for _ in range(4):
            m = np.arange(max(c - w, 0), min(c + w, N - 1) + 1)
            wt = np.maximum(q[m] - floor, 0)
            sw, sm = int(wt.sum()), int(((m - c) * wt).sum())
            cf = 256 * c + (floor_div(512 * sm + sw, 2 * sw) if sw else 0)
            c = (cf + 128) >> 8
        cen.append(cf)
    if plan["known"]:
        spacing = 64 * d
        f0 = floor_div(sum(cen) - 6 * spacing + 2, 4)
    else:
        s10 = -3 * cen[0] - cen[1] + cen[2] + 3 * cen[3]
        spacing = floor_div(s10 + 5, 10)
        f0 = floor_div(5 * sum(cen) - 3 * s10 + 10, 20)
    wf = w * floor
    quality = min(256 * (score - wf) // max(wf, 1), 0xFFFFFFFF) if score > wf else 0
    return dict(f0_q8=f0, spacing_q8=spacing, c0=c0, d=d, w=w, floor=floor, score=score, quality_q8=quality,
                valid=int(quality >= min_quality_q8 and bool(segments_ok)), centroid_q8=cen)


def record_dict(r):
    """A record of capi.FSK4_COMB_RECORD_DTYPE as comb_detect's dict."""
    d = {k: int(r[k]) for k in ("f0_q8", "spacing_q8", "c0", "d", "w", "floor", "score", "quality_q8", "valid")}
    d["centroid_q8"] = [int(v) for v in r["centroid_q8"]]
    return d


def f0_hz(rec, fsd):
    return (rec["f0_q8"] / 256.0 - 2048.0) * (fsd / 4096.0)


def spacing_hz(rec, fsd):
    return rec["spacing_q8"] / 256.0 * (fsd / 4096.0)


# ---- the object: epochs, decay, records, retunes

_SEGMENTS = {}


def segment_power(FT, x):
    """|X|^2 of one windowed segment, fftshifted, float64[4096]: the tone search's restatement on a fresh stream."""
    if "h" not in _SEGMENTS:
        _SEGMENTS["h"] = FT.HostFsk4Track(1.0, 0.001, 0.01, 0.02, -0.4, 0.4, epoch_segments=4096)      # (any search: its epoch never ends here)
    h = _SEGMENTS["h"]
    h.reset()
    h.push(x)
    return h.acc()


def steps(fsd, f0, spacing):
    return [int(np.rint((f0 + t * spacing) / fsd * 2.0 ** 32)) & 0xFFFFFFFF for t in range(4)]


def wants_retune(rec, phi, fsd, baud, deadband):
    if not rec["valid"]:
        return False
    for t in range(4):
        have = (phi[t] - (1 << 32) if phi[t] & 0x80000000 else phi[t]) / 4294967296.0 * fsd
        want = f0_hz(rec, fsd) + t * spacing_hz(rec, fsd)
        if abs(want - have) > deadband / 256.0 * baud:
            return True
    return False


def track(FT, iq, fsd, baud, spacing_lo, spacing_hi, f_lo, f_hi, modem_phi=None, **params):
    """The tracker over the samples since a reset: (records -- comb_detect's dicts with end_sample and epoch --, the sums at the end, the retunes
    [(at_sample, f0_hz, spacing_hz)] an attached modem with the steps modem_phi gets)."""
    p = dict(DEFAULTS, **params)
    plan = comb_plan(fsd, baud, spacing_lo, spacing_hi, f_lo, f_hi)
    assert isinstance(plan, dict), plan
    iq = np.ascontiguousarray(iq, np.complex64)
    acc, eff, keep = np.zeros(N, np.float64), 0.0, p["decay_q8"] / 256.0
    records, retunes, phi = [], [], None if modem_phi is None else list(modem_phi)
    E = p["epoch_segments"]
    for j in range(max(0, (iq.size - N) // HOP + 1) if iq.size >= N else 0):
        acc = acc + segment_power(FT, iq[HOP * j:HOP * j + N])
        if (j + 1) % E:
            continue
        eff += float(E)
        r = comb_detect(acc, plan, p["min_quality_q8"], eff >= p["min_segments"])
        acc = acc * keep
        eff *= keep
        r.update(end_sample=HOP * (j + 2), epoch=(j + 1) // E - 1)
        records.append(r)
        if phi is not None and wants_retune(r, phi, fsd, baud, p["deadband"]):
            f0, sp = f0_hz(r, fsd), spacing_hz(r, fsd)
            if all(abs(f0 + t * sp) < fsd / 2 for t in range(4)):
                retunes.append((r["end_sample"], f0, sp))
                phi = steps(fsd, f0, sp)
    return records, acc, retunes


# ---- the modem's retune (hd_fsk4_retune) on top of fsk4_model

def slot_records_retuned(iq, fsd, baud, f0, spacing, retunes=(), window_q8=256):
    """fsk4_model.slot_records with retunes [(at_sample, f0_hz, spacing_hz)], already in the order and at the samples at which they take effect:
    from at_sample on Phi_t are the new steps and Psi_t += at_sample (Phi_old - Phi_new) mod 2^32."""
    m = FM.modem(fsd, baud, f0, spacing, window_q8)
    iq = np.ascontiguousarray(iq, np.complex64)
    ends, g = [], 0
    while FM.slot_end(m["F"], g) < iq.size:
        ends.append(FM.slot_end(m["F"], g))
        g += 1
    ends = np.array(ends, np.int64)
    q_re, q_im = TM.quantise(iq.real), TM.quantise(iq.imag)
    i = np.arange(iq.size, dtype=np.uint64)
    phi = np.tile(np.array(m["step"], np.uint64)[:, None], (1, iq.size))
    psi = np.zeros((4, iq.size), np.uint64)
    cur_phi, cur_psi = list(m["step"]), [0, 0, 0, 0]
    for at, rf0, rsp in retunes:
        new = steps(fsd, rf0, rsp)
        for t in range(4):
            cur_psi[t] = (cur_psi[t] + at * (cur_phi[t] - new[t])) & 0xFFFFFFFF
            cur_phi[t] = new[t]
            phi[t, at:] = cur_phi[t]
            psi[t, at:] = cur_psi[t]
    out = np.zeros((ends.size, 4), np.uint32)
    for t in range(4):
        theta = ((i & np.uint64(0xFFFFFFFF)) * phi[t] + psi[t]) & np.uint64(0xFFFFFFFF)
        a = (theta >> np.uint64(22)).astype(np.int64)
        c, s = TM.C_TABLE[a], TM.C_TABLE[(a + 768) & 1023]
        r_re, r_im = (q_re * c + q_im * s) >> 15, (q_im * c - q_re * s) >> 15
        s_re, s_im = TM.window_sum(r_re, m["W"])[ends], TM.window_sum(r_im, m["W"])[ends]
        out[:, t] = TM.isqrt(s_re * s_re + s_im * s_im)
    return out


def receive_retuned(iq, fsd, baud, f0, spacing, fr, retunes=(), **kw):
    """fsk4_model.receive with retunes: (slot records, candidates behind the gate, frames, counters)."""
    slots = slot_records_retuned(iq, fsd, baud, f0, spacing, retunes)
    cands, decided = FM.candidates(slots, fr, kw.get("uw_max_errors", 2), kw.get("chase_bits", 4))
    frames, counters = FM.select(cands, fr, FM.modem(fsd, baud, f0, spacing)["F"], decided, kw.get("max_corrected"))
    return slots, cands, frames, counters


def effective(retunes, iq_size):
    """Retunes as hd_fsk4_retune's rules put them in force when all are queued before the first sample: in the order of the calls, each at its sample
    or, where the one in front of it came later, at that one's."""
    out, at_min = [], 0
    for at, f0, sp in retunes:
        at_min = max(at_min, at)
        if at_min < iq_size:
            out.append((at_min, f0, sp))
    return out


# ---- signals

FSD, BAUD = 32000.0, 1000.0                                          # 32 samples per symbol; one baud is 128 bins
SPACING = 2.7 * BAUD


def drifting_fsk4(syms, fs, baud, f0, spacing, drift_hz=0.0, sigma=0.0, seed=0, n_samples=None):
    """fsk4_model.fsk4_iq from sample 0 with all four tones moving linearly by drift_hz over the n samples."""
    syms = np.asarray(syms, np.int64)
    spb = fs / baud
    n = int(np.ceil(syms.size * spb)) if n_samples is None else int(n_samples)
    i = np.arange(n, dtype=np.float64)
    k = np.floor(i / spb).astype(np.int64)
    on = k < syms.size
    f = np.where(on, f0 + spacing * syms[np.clip(k, 0, syms.size - 1)] + drift_hz * i / n, 0.0)
    iq = np.where(on, np.exp(2j * np.pi * np.cumsum(f) / fs), 0.0)
    if sigma:
        rng = np.random.default_rng(seed)
        iq = iq + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return iq.astype(np.complex64)


def frames_signal(n_frames, f0, drift_hz=0.0, sigma=0.6, seed=5):
    """(iq, payloads): n_frames V1 frames back to back at 32 samples per symbol, spacing 2.7 baud, and one symbol time of noise behind them."""
    payloads = [FM.make_payload(FM.V1, 200 + k) for k in range(n_frames)]
    syms = np.concatenate([FM.symbols(FM.encode(p, FM.V1)) for p in payloads])
    n = int(syms.size * FSD / BAUD) + 2 * 4096                       # (the tail lets the last frame's contest end and the last epoch close)
    return drifting_fsk4(syms, FSD, BAUD, f0, SPACING, drift_hz, sigma, seed, n), payloads


def lobes(centres, width, level=1.0, base=0.0):
    """A built spectrum: `base` everywhere and a triangular lobe of `width` bins half-width and height `level` at every centre (bins, fractions allowed)."""
    k = np.arange(N, dtype=np.float64)
    acc = np.full(N, base, np.float64)
    for c in centres:
        acc += level * np.maximum(0.0, 1.0 - np.abs(k - c) / width)
    return acc


# ---- the accuracy ladder (tests/golden/fsk4_track_ladder.json, made by tools/gen_golden_fsk4_track.py) and the noise run

LADDER = dict(fsd=FSD, baud=BAUD, spacing=SPACING, sigmas=[0.6, 0.85, 1.0], segments=[2, 4, 8], trials=12, seed=20261021,
              spacing_lo=2.0 * BAUD, spacing_hi=3.5 * BAUD, f_lo=-9000.0, f_hi=9000.0)


def ladder_trial(g, sigma, segs, k):
    """(iq, the lowest tone sent): random symbols at 32 samples per symbol for `segs` segments, the tones somewhere in the band."""
    rng = np.random.default_rng([g["seed"], int(round(100 * sigma)), segs, k])
    f0 = -4050.0 + rng.uniform(-1500.0, 1500.0)
    n = HOP * (segs + 1)
    syms = rng.integers(0, 4, int(n * g["baud"] / g["fsd"]) + 1)
    return FM.fsk4_iq(syms, g["fsd"], g["baud"], f0, g["spacing"], sigma=sigma, seed=int(rng.integers(1 << 31)), n_samples=n), f0


def ladder_cell(g, sigma, segs, detect):
    """detect(iq, segs) -> the record of the one epoch of `segs` segments.  The worst error of each tone over the trials in baud, and the quality's range."""
    err, quality = [0.0] * 4, []
    for k in range(g["trials"]):
        iq, f0 = ladder_trial(g, sigma, segs, k)
        r = detect(iq, segs)
        for t in range(4):
            e = abs(f0_hz(r, g["fsd"]) + t * spacing_hz(r, g["fsd"]) - (f0 + t * g["spacing"])) / g["baud"]
            err[t] = max(err[t], e)
        quality.append(r["quality_q8"])
    return dict(sigma=sigma, segments=segs, err_baud=err, quality_min=min(quality), quality_max=max(quality))


def ladder(g, detect):
    return [ladder_cell(g, sigma, segs, detect) for sigma in g["sigmas"] for segs in g["segments"]]


def ladder_args(g):
    return (g["fsd"], g["baud"], g["spacing_lo"], g["spacing_hi"], g["f_lo"], g["f_hi"])


def model_detect(FT, g):
    return lambda iq, segs: track(FT, iq, *ladder_args(g), epoch_segments=segs, min_segments=segs)[0][0]


def host_detect(FT, g):
    def detect(iq, segs):
        h = FT.HostFsk4Track(*ladder_args(g), epoch_segments=segs, min_segments=segs)
        h.push(iq)
        return record_dict(h.records()[0]["rec"])
    return detect


NOISE = dict(sigma=1.0, epochs=200, epoch_segments=4, seed=77)


def noise_qualities(FT, g, nz=NOISE):
    """The quality of every epoch of noise alone, through the restatement (decay 0: every epoch on its own)."""
    rng = np.random.default_rng(nz["seed"])
    n = HOP * (nz["epochs"] * nz["epoch_segments"] + 1)
    iq = (nz["sigma"] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    h = FT.HostFsk4Track(*ladder_args(g), epoch_segments=nz["epoch_segments"], min_segments=nz["epoch_segments"], decay_q8=0, min_quality_q8=0)
    h.push(iq)
    r = h.records()
    assert len(r) == nz["epochs"]
    return [int(v) for v in r["rec"]["quality_q8"]]


# ---- the built spectra the detector's tests share: (name, sums, the search (baud, spacing_lo, spacing_hi, f_lo, f_hi), valid expected)

BIN = FSD / N
WIDE = (BAUD, 2.0 * BAUD, 4.0 * BAUD, -12000.0, 12000.0)


def built_spectra():
    centres = [1500.3 + 345.6 * t for t in range(4)]
    nan = lobes(centres, 100, 1.0, 0.01)
    nan[777] = np.nan
    plateaus = np.full(N, 0.01)
    for t in range(4):
        plateaus[1500 + 346 * t - 50:1500 + 346 * t + 51] = 1.0
    # the comb c0 = 1032, d = 1382 (centres + 0, 346, 691, 1037) with its first window's first bin and its last window's last bin on the band's edges:
    # with the spacing given it is the band's only candidate
    edge_band = (BAUD, 345.5 * BIN, 345.5 * BIN, (1000 - 2048) * BIN, (1032 + 1037 + 32 - 2048) * BIN)
    return [
        ("clean", lobes(centres, 100, 1.0, 0.01), WIDE, 1),
        ("edges", lobes([1032, 1032 + 346, 1032 + 691, 1032 + 1037], 24, 1.0, 0.01), edge_band, 1),
        ("three_of_four", lobes(centres[:2] + centres[3:], 100, 1.0, 0.01), WIDE, 0),
        ("carrier", lobes(centres[:1], 100, 1.0, 0.01), WIDE, 0),
        ("rtty_pair", lobes(centres[:2], 100, 1.0, 0.01), WIDE, 0),
        ("zeros", np.zeros(N), WIDE, 0),
        ("nan", nan, WIDE, 0),
        ("tie", plateaus, WIDE, 1),
        ("known_spacing", lobes(centres, 100, 1.0, 0.01), (BAUD, SPACING, SPACING, -12000.0, 12000.0), 1),
    ]
