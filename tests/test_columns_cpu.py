"""CPU side of the passed rays as selected columns (include/sart.h: sart_trace_columns_passed): the C-ABI names and the column
enum, sart_columns_len, columns_from_records (the definition the GPU tests hold the kernels to), the code object of the three
new kernels and the command line's --events."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import raytracer as R
from solaraxionraytracing_amd.__main__ import EVENT_COLUMNS, build_parser, check_scan_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_columns_len", "sart_trace_columns_passed", "sart_trace_columns_passed_device")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    lib = L.load_sart()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SART_SYMBOLS, name
        assert re.search(r"proc %s\*\(" % name, nim), name
        assert hasattr(lib, name), name
    assert lib.sart_abi_version() == 5


def _snake(field):
    return re.sub(r"(?<=[a-z])(?=[A-Z])|(?<=[A-Z])(?=[A-Z][a-z])", "_", field).upper()


def test_column_enum_is_the_word_order_of_the_record():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    enum = {k: int(v) for k, v in re.findall(r"\bSART_COL_([A-Z0-9_]+) = (\d+)\b", hdr)}
    assert enum.pop("COUNT") == 27 == L.COLUMN_COUNT
    assert enum.pop("RAY_ID") == 26 == L.COLUMNS["ray_id"]
    assert sorted(enum.values()) == list(range(26))                       # one name per 8-byte word of the 208-byte record
    assert _snake("pointdataXBefore") == "POINTDATA_X_BEFORE" and _snake("transProbWindow") == "TRANS_PROB_WINDOW"
    by_word = {}
    for name in L.AXION_DTYPE.names:
        by_word.setdefault(L.AXION_DTYPE.fields[name][1] // 8, name)     # the first field of a word names the two packed words
    assert by_word[0] == "passed" and by_word[16] == "kinds"
    for word, field in by_word.items():
        key = {"passed": "FLAGS", "kinds": "KINDS"}.get(field, _snake(field))
        assert enum[key] == word == L.AXION_DTYPE.fields[field][1] // 8, (field, key)
    assert len(by_word) == 26
    # the Python table: every 8-byte field by its word, the packed words and the ray id
    eight = [n for n in L.AXION_DTYPE.names if L.AXION_DTYPE.fields[n][0].itemsize == 8]
    assert set(L.COLUMNS) == set(eight) | {"flags", "kinds_packed", "ray_id"} and len(eight) == 24
    for n in eight:
        assert L.COLUMNS[n] == L.AXION_DTYPE.fields[n][1] // 8 == enum[_snake(n)]
    assert L.COLUMNS["flags"] == enum["FLAGS"] == 0 and L.COLUMNS["kinds_packed"] == enum["KINDS"] == 16
    assert sorted(L.COLUMNS.values()) == list(range(27))
    assert L.column_dtype("shellNumber") == np.int64 and L.column_dtype("weights") == np.float64
    assert all(L.column_dtype(n) == np.uint64 for n in ("flags", "kinds_packed", "ray_id"))
    assert L.column_mask(["weights", "ray_id", "flags"]) == (1 << 6) | (1 << 26) | 1
    with pytest.raises(KeyError):
        L.column_mask(["passed"])                                         # a byte of word 0: reached through "flags"


def test_columns_len_needs_no_device():
    f = L.load_sart().sart_columns_len
    assert f(0b1, 10) == 10 and f(1 << 26, 7) == 7 and f((1 << 27) - 1, 1000) == 27_000 and f(0x2062, 0) == 0
    assert f(L.column_mask(R.RayTracer.DEFAULT_COLUMNS), 123_457) == 6 * 123_457
    assert f(0, 10) == 0                                                  # no column
    assert f(1 << 27, 10) == 0 and f(0xFFFFFFFF, 10) == 0 and f((1 << 31) | 1, 10) == 0    # bits that name no column
    assert f(0b11, 1 << 63) == 0 and f((1 << 27) - 1, (1 << 64) // 27 + 1) == 0            # the product does not fit
    assert f(0b11, (1 << 63) - 1) == (1 << 64) - 2


def test_columns_from_records_on_hand_made_records():
    rec = np.zeros(3, dtype=L.AXION_DTYPE)
    raw = rec.view(np.uint8).reshape(3, 208)
    raw[:] = 0xEE                                                         # the padding bytes must not leak into the packed words
    doubles = [n for n in L.AXION_DTYPE.names if L.AXION_DTYPE.fields[n][0] == np.float64]
    assert len(doubles) == 23
    want_bits = {}
    for k in range(3):
        for j, n in enumerate(doubles):
            bits = np.uint64(0x3FF0_0000_0000_0000 + (k << 40) + (j << 8) + 0x5A)     # distinct in every word of every record
            rec[n][k] = np.array([bits]).view(np.float64)[0]
            want_bits[n, k] = bits
    rec["passed"], rec["passedTillWindow"], rec["hitNickel"] = [1, 0, 1], [1, 1, 0], [0, 1, 1]
    rec["kinds"], rec["kindsWindow"] = [3, 0, 250], [1, 7, 0]
    rec["shellNumber"] = [-1, 5, -(1 << 40)]
    ids = np.array([5, 9, (1 << 40) + 3], dtype=np.uint64)
    cols = R.columns_from_records(rec, list(L.COLUMNS), ray_ids=ids)
    assert list(cols) == sorted(L.COLUMNS, key=L.COLUMNS.get)             # ascending bit order, as the buffer holds them
    for n in doubles:
        assert cols[n].dtype == np.float64 and cols[n].flags.c_contiguous
        assert cols[n].view(np.uint64).tolist() == [int(want_bits[n, k]) for k in range(3)]
    assert cols["flags"].dtype == np.uint64 and cols["flags"].tolist() == [0x000101, 0x010100, 0x010001]
    assert cols["kinds_packed"].dtype == np.uint64 and cols["kinds_packed"].tolist() == [0x0103, 0x0700, 0x00FA]
    assert cols["shellNumber"].dtype == np.int64 and cols["shellNumber"].tolist() == [-1, 5, -(1 << 40)]
    assert cols["ray_id"].dtype == np.uint64 and cols["ray_id"].tolist() == ids.tolist()
    # a record whose padding is zero, as the library writes it: the packed columns are words 0 and 16 of its bytes
    raw[:, 3:8] = 0
    raw[:, 130:136] = 0
    words = raw.view("<u8").reshape(3, 26)
    for n, bit in L.COLUMNS.items():
        if n != "ray_id":
            assert cols[n].view(np.uint64).tolist() == words[:, bit].tolist(), n
    few = R.columns_from_records(rec, ("weights", "pointdataX", "weights"))
    assert list(few) == ["pointdataX", "weights"]
    with pytest.raises(ValueError):
        R.columns_from_records(rec, ("ray_id",))
    assert R.columns_from_records(rec[:0], ("weights",))["weights"].shape == (0,)


def _kernel_blocks(tmp_path):
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    out = {}
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if m and re.search(r"columns_(stage|count|scatter)_kernel", m.group(1)):
            out[m.group(1)] = k
    return out


def test_column_kernels_meet_the_ray_kernel_budgets(tmp_path):
    """One kernel each, named without `trace_` (tests/test_host_and_abi.py counts those); the stage kernel keeps the record in
    registers: no scratch, no spills, at most 128 VGPRs."""
    blocks = _kernel_blocks(tmp_path)
    assert len(blocks) == 3 and all("trace_" not in n for n in blocks), sorted(blocks)
    for which in ("stage", "count", "scatter"):
        assert sum("columns_%s_kernel" % which in n for n in blocks) == 1, which
    g = lambda k, key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
    for name, k in blocks.items():
        assert g(k, "private_segment_fixed_size") == 0 and g(k, "vgpr_spill_count") == 0, name
        assert g(k, "vgpr_count") <= 128, (name, g(k, "vgpr_count"))


def _parse(argv):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_scan_args(ap, args)
    return args


def test_cli_accepts_events():
    a = _parse(["--events", "ev.npz"])
    assert a.events == "ev.npz" and tuple(a.eventColumns.split(",")) == EVENT_COLUMNS
    assert EVENT_COLUMNS == ("pointdataX", "pointdataY", "pointdataR", "energiesAx", "weights", "shellNumber", "ray_id")
    assert _parse(["--events", "ev.npz", "--eventColumns", "weights, flags"]).eventColumns == "weights, flags"
    assert _parse(["--events", "ev.npz", "--shellBreakdown"]).shellBreakdown
    assert _parse([]).events == ""


@pytest.mark.parametrize("extra", [["--massScanMin", "0", "--massScanMax", "0.02"],
                                   ["--angularScanMin", "0", "--angularScanMax", "0.1"],
                                   ["--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8"]])
def test_cli_refuses_events_beside_a_scan(extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--events", "ev.npz"] + extra)
    assert e.value.code == 2
    assert "cannot be combined" in capsys.readouterr().err


def test_cli_refuses_unknown_event_columns(capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--events", "ev.npz", "--eventColumns", "weights,passed"])
    assert e.value.code == 2 and "passed" in capsys.readouterr().err
