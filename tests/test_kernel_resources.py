"""The register / scratch claims of DESIGN.md, checked from the compiler's own metadata (no GPU needed: hipcc cross-compiles a device-only listing).

k_step_cu and k_stage1_cu must not spill and must keep the occupancy their launch shapes assume: two waves per SIMD for the 512-thread step workgroup
(<= 256 VGPRs), four for the 1024-thread-capable stage-1 workgroup (<= 128)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "habdec_amd" / "csrc"


def kernel_table(src: Path, tmp: Path, fast: bool = False):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp / (src.stem + ".s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
           "-I", str(ROOT / "include"), "-I", str(CSRC), *(["-DHD_FAST_ARITH"] if fast else []), "-x", "hip", "--cuda-device-only", "-S", str(src), "-o", str(out)]
    try:
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    except subprocess.CalledProcessError as ex:              # a hipcc that cannot target gfx950: nothing to check here
        pytest.skip("hipcc could not produce a gfx950 listing: " + ex.stderr.decode(errors="replace")[-400:])
    except subprocess.TimeoutExpired:
        pytest.skip("hipcc did not finish the gfx950 listing within 900 s")
    txt = out.read_text()
    meta = txt[txt.index("amdhsa.kernels:"):]
    table = {}
    for blk in re.split(r"\n  - \.agpr_count", meta)[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        name = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*", "", name).replace("void hd::", "").replace("hd::", "").replace("exact::", "").replace("fast::", "").replace(" ", "")
        table[name] = dict(vgpr=int(g("vgpr_count")), spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                           sgpr=int(g("sgpr_count")), sgpr_spill=int(g("sgpr_spill_count")), lds=int(g("group_segment_fixed_size")))
    return table


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_step_and_stage1_kernels_do_not_spill(tmp_path, fast):
    """(both arithmetic modes: the translation unit is compiled once per mode, kernels/arith.h)"""
    t = kernel_table(CSRC / "kernels" / "decimate.hip", tmp_path, fast)
    if fast:       # the fast mode's FIR loops are fused multiply-adds: the listing must carry them, and the exact mode's must not
        txt = (tmp_path / "decimate.s").read_text()
        assert txt.count("v_pk_fma_f32") > 2000, txt.count("v_pk_fma_f32")
    else:
        assert (tmp_path / "decimate.s").read_text().count("v_pk_fma_f32") == 0
    for k in ("k_step_cu<212,2,69>", "k_step_cu<174,4,139>"):
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 256, (k, t[k])
    for k in ("k_stage1_cu<212,32>", "k_stage1_cu<174,32>"):
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 128, (k, t[k])
    # (/8: all 54 taps live in scalar registers; the compiler parks a few scalars in vector lanes and keeps a 20-byte frame for them that no
    # instruction of the kernel touches -- no vector spills, no scratch_ instruction in the listing)
    k = "k_stage1_cu<54,8>"
    assert t[k]["spill"] == 0 and t[k]["scratch"] <= 32 and t[k]["vgpr"] <= 256, (k, t[k])
    # the single-wave fallback of the step launch: no spills either (round 6: its tile loader's loop-invariant lane masks no longer live in scalar
    # registers across the tile loop -- 12 bytes of scratch and 256 registers before)
    for k in ("k_step<32,212,2,69>", "k_step<32,174,4,139>"):
        assert t[k]["spill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 256, (k, t[k])
    # the DC blocker's 64-lane recurrence: a handful of registers, nothing spilled (fully unrolled it had parked 130 scalars)
    assert t["k_dc_remove"]["spill"] == 0 and t["k_dc_remove"]["scratch"] == 0 and t["k_dc_remove"]["vgpr"] <= 32, t["k_dc_remove"]
