"""Writes tests/golden/fsk4_track_ladder.json: the 4FSK tone tracker's accuracy ladder from the numpy model (tests/fsk4_track_model.py) -- per noise level
and number of segments the worst error of each of the four tones over the trials, in baud, and the quality's range.  tests/test_fsk4_track_host.py holds
the host restatement to this file.

    python tools/gen_golden_fsk4_track.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import fsk4_track_model as M  # noqa: E402
from habdec_amd.build import build  # noqa: E402

if __name__ == "__main__":
    build()
    from habdec_amd import fsk4_track as FT
    out = dict(M.LADDER, cells=M.ladder(M.LADDER, M.model_detect(FT, M.LADDER)))
    path = ROOT / "tests" / "golden" / "fsk4_track_ladder.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    for c in out["cells"]:
        print(c["sigma"], c["segments"], " ".join(f"{e:.3f}" for e in c["err_baud"]), c["quality_min"], c["quality_max"])
