"""Writes tests/golden/fsk4_ladder.json: the 4FSK sensitivity ladder's signal parameters, one seed per rung, and the frames the numpy MODEL
(tests/fsk4_model.py) delivers on each rung at chase_bits 0 and 4.  tests/test_fsk4_host.py holds the host restatement to these counts.

The rungs run from every frame delivered to none; no Eb/N0 figure is fixed in advance -- the sigmas only have to span that range.

    python3 tools/gen_golden_fsk4.py"""
import json
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import fsk4_model as FM

# 8 samples per symbol, amplitude 1, noise sigma per component: Es/N0 = 8 / (2 sigma^2); per information bit (176 payload bits in 180 symbols) Eb/N0 = Es/N0 * 180 / 176
g = dict(preset=1, fsd=32000.0, baud=4000.0, f0=-6000.0, spacing=4000.0, frames=12, gap=560, rungs=[])
fr = FM.V1
for k, sigma in enumerate((0.6, 0.8, 0.85, 0.9, 0.95, 1.0, 1.05, 1.2)):
    rung = dict(sigma=sigma, seed=900 + k)
    iq, payloads = FM.ladder_signal(g, rung)
    for chase in (0, 4):
        frames = FM.receive(iq, g["fsd"], g["baud"], g["f0"], g["spacing"], fr, chase_bits=chase)[2]
        assert all(f["payload"] in payloads for f in frames), "a frame nobody sent"
        rung["delivered_chase%d" % chase] = len(frames)
    print(rung, flush=True)
    g["rungs"].append(rung)
(ROOT / "tests" / "golden" / "fsk4_ladder.json").write_text(json.dumps(g, indent=1) + "\n")
