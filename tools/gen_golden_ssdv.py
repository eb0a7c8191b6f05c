"""Writes tests/golden/ssdv_ladder_s3_028.records and .packets: the clocked restatement's records of the SSDV ladder's row of seed 3 at sigma 0.28
(tests/ssdv_model.ladder_row -> hd_host_clocked_*), as hd_clocked_record structs, and the six packets that were sent.  tools/ssdv_host_check.cpp reads
them, so that the sanitizer run covers a real ladder row without numpy.

    python3 tools/gen_golden_ssdv.py"""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import habdec_amd
import ssdv_model as SM

row, sent = SM.ladder_row(3, 0.28)
hc = habdec_amd.HostClocked(8000.0, baud=300.0, bits=8, stops=2)
hc.push(row)
rec = hc.records()
out = ROOT / "tests" / "golden"
(out / "ssdv_ladder_s3_028.records").write_bytes(rec.tobytes())
(out / "ssdv_ladder_s3_028.packets").write_bytes(b"".join(sent))
print(len(rec), "records,", len(sent), "packets")
