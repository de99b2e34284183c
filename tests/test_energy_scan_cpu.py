"""CPU side of the fused energy scan (include/sart.h: sart_trace_energy_scan): the C-ABI tables, the Nim binding, the code object
of energy_scan_kernel and the command line's new switches."""
import os
import re
import shutil
import subprocess

import pytest

from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd.__main__ import build_parser, check_scan_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_trace_energy_scan_device", "sart_trace_energy_scan", "sart_finalize_energy_scan_device", "sart_energy_scan_len")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    lib = L.load_sart()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SART_SYMBOLS, name
        assert re.search(r"proc %s\*" % name, nim), name
        assert hasattr(lib, name), name
    assert lib.sart_abi_version() == 5


def test_layout_constants_agree_across_header_library_and_python():
    hdr = open(os.path.join(ROOT, "include", "sart.h")).read()
    for key, slot in list(L.ESCAN.items()) + [(k + "_HI", v) for k, v in L.ESCAN_HI.items()]:
        assert re.search(r"SART_ESCAN_%s = %d\b" % (key, slot), hdr), key
    for key, slot in L.ESCAN_SHARED.items():
        assert re.search(r"SART_ESCAN_%s = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_ESCAN_ROW = %d\b" % L.ESCAN_ROW, hdr)
    lib = L.load_sart()
    for n in (1, 7, 32, 33, 99):
        assert lib.sart_energy_scan_len(n) == L.energy_scan_len(n) == (n + 1) * 8
    rows, shared = L.split_energy_scan(list(range(L.energy_scan_len(2))), 2)
    assert list(rows["N_PASSED_TILL_WINDOW"]) == [3, 11] and shared["N_HIT_NICKEL"] == 19.0


def _kernel_blocks(tmp_path):
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    out = []
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if m and "energy_scan_kernel" in m.group(1):
            out.append((m.group(1), k))
    return out


def test_energy_scan_kernel_meets_the_ray_kernel_budgets(tmp_path):
    """No scratch, <= 128 VGPRs (four waves per SIMD at 1024 threads), LDS within 160 KB - for all four instantiations
    ({not rotated, rotated} x {f64, FIXED64})."""
    blocks = _kernel_blocks(tmp_path)
    assert len(blocks) == 4, [n for n, _ in blocks]
    for name, k in blocks:
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        assert g("vgpr_count") <= 128, (name, g("vgpr_count"))
        assert g("group_segment_fixed_size") <= 160 * 1024, (name, g("group_segment_fixed_size"))
        assert g("kernarg_segment_size") <= 4096, name


def _parse(argv):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_scan_args(ap, args)
    return args


def test_cli_accepts_the_energy_scan_switches():
    a = _parse(["--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8", "--numEnergyScanPoints", "15"])
    assert (a.energyScanMin, a.energyScanMax, a.numEnergyScanPoints) == (1.0, 8.0, 15)
    assert _parse([]).numEnergyScanPoints == 32


@pytest.mark.parametrize("extra", [["--massScanMin", "0", "--massScanMax", "0.02"],
                                   ["--angularScanMin", "0", "--angularScanMax", "0.1"]])
def test_cli_refuses_the_energy_scan_beside_another_scan(extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8"] + extra)
    assert e.value.code == 2
    assert "cannot be combined" in capsys.readouterr().err


@pytest.mark.parametrize("bad", [["--energyScanMin", "5", "--energyScanMax", "1"], ["--energyScanMin", "-1", "--energyScanMax", "1"],
                                 ["--energyScanMin", "1", "--energyScanMax", "2", "--numEnergyScanPoints", "0"]])
def test_cli_refuses_an_empty_energy_range(bad):
    with pytest.raises(SystemExit) as e:
        _parse(["--xrayTest"] + bad)
    assert e.value.code == 2


def test_cli_refuses_the_energy_scan_without_the_test_source(tmp_path):
    """Exit 2 before any GPU work: the solar source has no energy scan."""
    from solaraxionraytracing_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--energyScanMin", "1", "--energyScanMax", "8", "--outpath", str(tmp_path)])
    assert e.value.code == 2
    assert not os.path.exists(tmp_path / "energy_scan.csv")
