"""tests/golden/afsk_ladder.json: what the numpy model (tests/afsk_model.py) makes of one UI frame under white noise on the row, a few seeds per level.

    python tools/gen_golden_afsk.py

Per seed: plain / repaired / lost, and the flips.  tests/test_afsk_host.py replays the same rows through the host restatement.  The levels reach from
where every frame decodes plain to where every one is lost; the audio's peak is 0.5."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import afsk_cases as K                     # noqa: E402
from afsk_model import AfskModel           # noqa: E402

SIGMAS = (0.25, 0.35, 0.40, 0.45, 0.70)
SEEDS = 5
HEAD = dict(info=K.INFO.decode("latin-1"), max_frame_bytes=64, start=300.25)


def main():
    f = K.ui_frame(K.INFO)
    clean = K.row_of(K.nrzi(K.on_air([f])), K.BELL, dict(max_frame_bytes=HEAD["max_frame_bytes"]), start=HEAD["start"])
    levels = []
    for li, sigma in enumerate(SIGMAS):
        runs = []
        for k in range(SEEDS):
            seed = 1000 * li + k
            row = (clean + sigma * np.random.default_rng(seed).standard_normal(clean.size)).astype(np.float32)
            m = AfskModel(K.FS, *K.BELL, max_frame_bytes=HEAD["max_frame_bytes"])
            m.push(row)
            got = [fr for fr in m.take_frames() if fr["data"] == f[:-2]]
            runs.append(dict(seed=seed, outcome="lost" if not got else "repaired" if got[0]["flips"] else "plain", flips=got[0]["flips"] if got else 0))
        print(sigma, [r["outcome"] for r in runs])
        levels.append(dict(sigma=sigma, runs=runs))
    out = ROOT / "tests" / "golden" / "afsk_ladder.json"
    out.write_text(json.dumps(dict(HEAD, levels=levels), indent=1) + "\n")
    print(out)


if __name__ == "__main__":
    main()
