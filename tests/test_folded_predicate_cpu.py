"""The host's rule for the folded kernel form (csrc/sart_device.h: folded_form_applies, through the test entry
sart_internal_folded_form_applies of libsart; no device needed) as a truth table over its inputs: the folded form is taken for the
one combination in which every folded answer holds, and for no other; and the code object holds the folded kernels within the
budget of the other histogram kernels (no scratch, at most 128 VGPRs, the same LDS)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

from solaraxionraytracing_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the inputs in the entry's order, each with its folded answer first and then answers that are not
INPUTS = [
    ("constant_path", (1, 0)),
    ("records_on", (1, 0)),
    ("radial_table", (1, 0)),
    ("zones", (1, 0)),
    ("xmm", (1, 0)),
    ("spoke_n", (16, 6, 0, 17)),
    ("n_half_strips", (2, 0, 1, 3, 16)),
    ("flags", (0, L.CF_IGNORE_DET_WINDOW, L.CF_IGNORE_GAS_ABS, L.CF_IGNORE_REFLECTION, L.CF_IGNORE_CONV_PROB, L.CF_XRAY_TEST,
               L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB)),
    ("spectra", (0, 1)),
    ("no_folded", (0, 1)),
]


def applies(values):
    fn = L.load_sart().sart_internal_folded_form_applies
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32)]
    got = fn((C.c_uint32 * len(values))(*values))
    assert got in (0, 1)
    return got


def test_every_folded_answer_gives_the_folded_form():
    assert applies([v[0] for _, v in INPUTS]) == 1


def test_flags_that_are_not_folded_do_not_matter():
    base = [v[0] for _, v in INPUTS]
    k = [n for n, _ in INPUTS].index("flags")
    for f in (L.CF_READ_MAGNET_CONFIG, L.CF_READ_DET_INSTALL_CONFIG, L.CF_READ_MAGNET_CONFIG | L.CF_READ_DET_INSTALL_CONFIG, 0x40000000):
        assert applies(base[:k] + [f] + base[k + 1:]) == 1, hex(f)
        assert applies(base[:k] + [f | L.CF_IGNORE_REFLECTION] + base[k + 1:]) == 0, hex(f)


def test_truth_table():
    """The whole product of the answers above (17920 rows): folded if and only if every input has its folded answer."""
    n = 0
    for row in itertools.product(*(v for _, v in INPUTS)):
        want = all(x == v[0] for x, (_, v) in zip(row, INPUTS))
        assert applies(list(row)) == int(want), dict(zip((k for k, _ in INPUTS), row))
        n += 1
    assert n == 17920


def test_folded_kernels_stay_within_the_histogram_kernels_budget(tmp_path):
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    llvm = "/opt/rocm/lib/llvm/bin"
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    want = (C.c_int32 * 8)()
    L.load_sart().sart_internal_kernarg_layout(want)
    seen = 0
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if not m or "folded_histogram_kernel" not in m.group(1):
            continue
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, m.group(1)
        assert g("vgpr_count") <= 128, (m.group(1), g("vgpr_count"))
        assert 160 * 1024 - 4096 < g("group_segment_fixed_size") <= 160 * 1024, g("group_segment_fixed_size")
        # the argument offsets the reload helpers read at (tests/test_host_and_abi.py holds trace_histogram_kernel to the same)
        args = re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)", k)
        explicit = [(int(o), int(sz)) for o, sz, kind in args if not kind.startswith("hidden")]
        assert [o for o, _ in explicit] == list(want[:6]), (m.group(1), explicit, list(want))
        seen += 1
    assert seen == 4   # vacuum and gas, f64 and FIXED64
