"""The loop control of trace_histogram_kernel with the wide pass of stage A0 (csrc/sart_trace_histogram.inc) as a Python model,
against a model of the one-word loop; the host's rule for switching it on (csrc/sart_api.hip: a0_wide_rule) against the same model;
and the budgets of the compiled kernels.  No GPU.

The models follow the kernel statement by statement for ONE wave: chunks of 256 ids, lane l owns ids 4l .. 4l + 3 of a chunk and
takes them in passes 0 .. 3; ring 0 (128 slots) between stage A0 and stage A1, ring 1 (128 slots) between stage A1 and phase B; 64
entries leave a ring whenever it holds as many, the rest when the input is exhausted.  What a ray's fate is (dead in a zone and
counted as reached, dead and not counted, handed on; kept by stage A1 or not) is a fixed random property of its id."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_QUEUE = 128
SURVIVALS = (0.0, 0.05, 0.3, 0.488, 0.7, 0.95, 1.0)
KNOBS = (0, 1, 2)
MAX_SHARE = 0.125   # csrc/sart_api.hip: kA0WideMaxShare


def lib_fns():
    lib = L.load_sart()
    share, rule = lib.sart_internal_a0_wide_share, lib.sart_internal_a0_wide_rule
    share.restype, share.argtypes = C.c_double, [C.c_double]
    rule.restype, rule.argtypes = C.c_int, [C.c_double]
    return share, rule


def wide_for(knob, survival):
    """HotA::zone_reached's switch (kA0WideMask) as sync_blob sets it for SART_A0_WIDE = knob (zones exist in every case of the model)."""
    if knob == 0:
        return False
    return True if knob == 2 else bool(lib_fns()[1](survival))


class Fates:
    """Per id of n_chunks chunks: 0 handed on by stage A0, 1 dead and counted as reached, 2 dead; and whether stage A1 keeps it."""
    def __init__(self, n_chunks, survival, seed):
        rng = np.random.default_rng(seed)
        n = n_chunks * 256
        self.a0 = np.where(rng.random(n) < survival, 0, rng.integers(1, 3, n)).astype(np.int8)
        self.a1_keeps = rng.random(n) < 0.6


def run_loop(f, n_chunks, rel_begin, rel_end, wide, wave=0, waves_total=1):
    """The persistent loop of one wave.  Returns the batches stage A1 popped, the batches phase B popped, n_reached, the number of
    even passes that tried a second word and of those that fell back.  Asserts the invariants of the rings on the way."""
    ring0, ring1 = [], []
    a1_batches, b_batches = [], []
    n_reached = even_wide = fallbacks = 0
    seen = np.zeros(n_chunks * 256, dtype=np.int32)
    chunk, pas, it = wave, 0, 0
    lane4 = 4 * np.arange(64)

    def a0_word(rel, room):
        nonlocal n_reached
        valid = (rel >= rel_begin) & (rel < rel_end)
        fate = f.a0[rel]
        mask = valid & (fate == 0)
        if int(mask.sum()) > room:
            return False
        n_reached += int((valid & (fate == 1)).sum())
        seen[rel[valid]] += 1
        ring0.extend(rel[mask].tolist())   # in lane order: prefix_from(mask, t0)
        return True

    while True:
        it += 1
        assert it <= 4 * n_chunks + 8, "the loop ends: every iteration with input takes at least one word, the drain at least one entry"
        if chunk < n_chunks:
            assert len(ring0) <= 64, "n0 <= 64 at the entry of a pass"
            rel = chunk * 256 + pas + lane4
            assert a0_word(rel, K_QUEUE)
            if wide and not (pas & 1):
                even_wide += 1
                if a0_word(rel + 1, K_QUEUE - len(ring0)):
                    pas += 1
                else:
                    fallbacks += 1
            pas = (pas + 1) & 3
            if pas == 0:
                chunk += waves_total
            assert len(ring0) <= K_QUEUE, "ring 0 never holds more than its 128 slots"
        n0 = len(ring0)
        a1_due = n0 >= 64
        if chunk >= n_chunks:
            a1_due = n0 > 0
        if a1_due:
            batch, ring0[:] = ring0[:64], ring0[64:]
            a1_batches.append(batch)
            ring1.extend(r for r in batch if f.a1_keeps[r])
            assert len(ring1) <= K_QUEUE
        n1 = len(ring1)
        b_due, draining = n1 >= 64, False
        if chunk >= n_chunks:
            draining = not ring0
            b_due = b_due or (draining and n1 > 0)
        if b_due:
            b_batches.append(ring1[:64])
            ring1[:] = ring1[64:]
        if draining and not ring1:
            break
    own = np.zeros(n_chunks * 256, dtype=bool)       # the ids of this wave's chunks inside the launch
    for c in range(wave, n_chunks, waves_total):
        own[c * 256:(c + 1) * 256] = True
    own[:rel_begin] = False
    own[rel_end:] = False
    assert (seen == own).all(), "every valid id is taken by stage A0 exactly once, no other id at all"
    return a1_batches, b_batches, n_reached, even_wide, fallbacks


def check_case(n_chunks, survival, knob, cut_begin, last_holds, seed, wave=0, waves_total=1):
    rel_begin, rel_end = cut_begin, (n_chunks - 1) * 256 + last_holds
    if rel_begin >= rel_end:
        return None
    f = Fates(n_chunks, survival, seed)
    old = run_loop(f, n_chunks, rel_begin, rel_end, False, wave, waves_total)
    new = run_loop(f, n_chunks, rel_begin, rel_end, wide_for(knob, survival), wave, waves_total)
    assert new[0] == old[0], "stage A1 gets the same batches of ring entries in the same order"
    assert new[1] == old[1], "phase B gets the same batches"
    assert new[2] == old[2], "n_reached"
    assert all(len(b) == 64 for b in old[0][:-1]) and all(len(b) == 64 for b in old[1][:-1])
    return new


# the first chunk loses its first 0, 1 or 255 ids (ray_id_offset & 255; 256 is the next chunk's 0), the last one holds 1, 255 or all
# 256 of its ids (cut 255, 1 and 0 = 256 ids in)
CUTS = [(b, e) for b in (0, 1, 255) for e in (1, 255, 256)]


@pytest.mark.parametrize("n_chunks", (1, 2, 3))
@pytest.mark.parametrize("survival", SURVIVALS)
def test_small_launches_hand_phase_a_the_same_batches(n_chunks, survival):
    for knob in KNOBS:
        for cut_begin, last_holds in CUTS:
            check_case(n_chunks, survival, knob, cut_begin, last_holds, seed=11 * n_chunks + knob)


@pytest.mark.parametrize("survival", SURVIVALS)
def test_long_launches_hand_phase_a_the_same_batches(survival):
    for knob in KNOBS:
        for cut_begin, last_holds in ((0, 256), (255, 1), (1, 255)):
            check_case(501, survival, knob, cut_begin, last_holds, seed=7 + knob)
        check_case(501, survival, knob, 1, 255, seed=3, wave=1, waves_total=3)   # a wave among others: every third chunk


def chain_share(s):
    """The stationary share of fall-backs among the even passes: the Markov chain of ring 0's fill stated at a0_wide_fallback_share
    (sart_api.hip), written out again with numpy."""
    from math import comb
    pmf = np.array([comb(64, k) * s ** k * (1.0 - s) ** (64 - k) for k in range(65)])
    pop = lambda x: x - 64 if x >= 64 else x
    T, F = np.zeros((65, 65)), np.zeros(65)
    for n in range(65):
        for a in range(65):
            for b in range(65):
                p = pmf[a] * pmf[b]
                if n + a + b <= K_QUEUE:
                    T[n, pop(n + a + b)] += p
                else:
                    F[n] += p
                    T[n, pop(pop(n + a) + b)] += p
    pi = np.full(65, 1.0 / 65)
    for _ in range(20000):
        nxt = pi @ T
        done = np.abs(nxt - pi).sum() < 1e-13
        pi = nxt
        if done:
            break
    return float(pi @ F)


def test_the_hosts_rule_keeps_the_fall_backs_below_its_bound():
    share, rule = lib_fns()
    # the library's chain is the model's chain
    for s in (0.05, 0.3, 0.45, 0.488, 0.52, 0.6, 0.7, 0.95):
        assert share(s) == pytest.approx(chain_share(s), abs=1e-9), s
    assert share(0.0) == 0.0 and share(1.0) == pytest.approx(1.0, abs=1e-9)
    # the rule is the bound, the share grows with the survival rate, and the rule switches once
    grid = [k / 200.0 for k in range(201)]
    shares = [share(s) for s in grid]
    assert all(b >= a - 1e-12 for a, b in zip(shares, shares[1:]))
    for s, sh in zip(grid, shares):
        assert bool(rule(s)) == (sh <= MAX_SHARE), s
    assert rule(0.488) and rule(0.5) and not rule(0.6) and not rule(0.7) and not rule(1.0)
    assert share(0.488) == pytest.approx(0.021, abs=1e-3) and share(0.7) == pytest.approx(0.4, abs=1e-3)
    # and the chain is the loop: 4000 chunks = 8000 even passes.  A share p counted over N passes has the standard deviation
    # sqrt(p (1 - p) / N) if the passes were independent: 0.0016 at p = 0.021, 0.0055 at p = 0.4; the ring's fill correlates
    # neighbouring passes over a few tens of passes, so five times that is allowed.
    for s in (0.3, 0.488, 0.55, 0.7):
        new = check_case(4000, s, 2, 0, 256, seed=99)
        p, n = share(s), new[3]
        assert n == 8000   # two even passes per chunk, fall-back or not
        assert abs(new[4] / n - p) <= 5.0 * max((p * (1.0 - p) / n) ** 0.5, 1.0 / n) * 5.0 ** 0.5 + 1e-12, (s, new[4] / n, p)
    # wherever the rule says yes, the loop's own share stays below the bound the derivation states
    for s in (0.05, 0.3, 0.45, 0.488, 0.52, 0.55):
        if rule(s):
            new = check_case(2000, s, 1, 0, 256, seed=5)
            assert new[4] <= MAX_SHARE * new[3], s


def test_histogram_kernels_keep_their_budgets():
    """Every instantiation of the two kernels that compile the loop: at most 128 VGPRs (four waves per SIMD at 1024 threads), no
    scratch, no vector spills, LDS within 160 KB."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    obj = os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o")
    ks = [k for k in kr.kernels(kr.code_object_notes(obj)) if "trace_histogram_kernel" in k["name"] or "mass_scan_spectra_kernel" in k["name"]]
    assert len(ks) >= 30, len(ks)
    for k in ks:
        assert k["vgpr"] <= 128, k
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert 0 < k["lds"] <= 160 * 1024, k
