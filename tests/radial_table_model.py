"""Numpy restatement of the radial verdict table of the solar-source histogram kernels (csrc/sart_device.h: RadialLds; sart_api.hip:
build_radial_table; sart_kernels.hip: radial_verdict_table / radial_verdict_compares).  Shared by test_radial_table_cpu.py and
test_gpu_radial_table.py; no test of its own.

A verdict is one byte, code << 6 | shell: code 0 not selected, 1 selected and below shell0_miss_radius, 2 selected, 3 selected and
above mirror_miss_radius."""
import numpy as np

TK_LLNL, TK_XMM, TK_ABRIXAS = 0, 1, 3
LUT_MAX, TABLE_MAX, MARKED = 1024, 128, 255


class Geo:
    """What the radial verdicts depend on.  shell0_miss: DevParams::shell0_miss_radius (-1: off); mirror_miss: mirror_miss_radius as the
    float the device holds (inf: off); fine_step: the look-up table's step as hoist_setup chooses it with the table on."""

    def __init__(self, setup, shell0_miss=-1.0, mirror_miss=np.inf, rotated=False, fine_step=True):
        n = int(setup.n_shells)
        self.kind = int(setup.telescope_kind)
        self.r1 = np.array(setup.all_r1[:n], dtype=np.float64)
        self.ro = self.r1 + np.array(setup.all_thickness[:n], dtype=np.float64)
        self.n = n
        self.inner, self.ring_lo, self.ring_hi = {TK_XMM: (64.7, 151.6 - 20.9, 151.6), TK_ABRIXAS: (37.5, 0.0, 0.0)}.get(self.kind, (0.0, 0.0, 0.0))
        self.shell0_miss = float(shell0_miss)
        self.mirror_miss = float(np.float32(mirror_miss)) if np.isfinite(mirror_miss) else np.inf
        self.cand_on = (not rotated) and self.kind != TK_LLNL
        self.r_last = float(self.r1[-1])
        # the look-up table of the shell selection (hoist_setup)
        min_gap = min(float(self.r1[0]), float(np.diff(self.r1).min())) if n > 1 else float(self.r1[0])
        step = min(1.0, 0.5 * min_gap)
        if fine_step:
            b = list(self.r1) + list(self.ro)
            if self.kind != TK_LLNL:
                b.append(self.inner)
            if self.kind == TK_XMM:
                b += [self.ring_lo, self.ring_hi]
            d = np.diff(np.sort(np.array(b)))
            for g in d[d > 1e-6]:
                step = min(step, 0.9 * float(g))
        step = max(step, self.r_last / (LUT_MAX - 2))
        assert step < min_gap
        self.step, self.inv_step = step, 1.0 / step
        self.lut_n = int(self.r_last / step) + 2
        lo = np.maximum(0.0, (np.arange(self.lut_n) - 1e-9) * step)
        self.lut = np.searchsorted(self.r1, lo, side="right").astype(np.int64)   # R1 ascending: the first shell with R1 > lo

    def cell(self, r):
        """max(min((int)(r * inv_step), lut_n - 1), 0) with the device's conversion: saturating, NaN -> 0."""
        with np.errstate(invalid="ignore", over="ignore"):
            x = np.asarray(r, dtype=np.float64) * self.inv_step
            x = np.where(x >= 0.0, np.minimum(x, float(self.lut_n - 1)), 0.0)   # NaN and negatives -> 0
        return np.trunc(x).astype(np.int64)

    def by_compares(self, r):
        """Today's predicate: phase_a_telescope's radial compares and the two sure-miss compares of stage A1."""
        r = np.atleast_1d(np.asarray(r, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            ok = np.ones(r.shape, dtype=bool)
            if self.kind != TK_LLNL:
                inner = (r <= self.inner) if self.kind == TK_XMM else (r < self.inner)
                ring = (r < self.ring_hi) & (r > self.ring_lo) if self.kind == TK_XMM else np.zeros(r.shape, dtype=bool)
                ok = ~(inner | ring)
            ok &= ~(r > self.r_last)
            nS = self.n
            j0 = self.lut[self.cell(r)]
            jc = np.minimum(j0, nS - 1)
            jb = np.maximum(jc - 1, 0)
            c_r1, c_ro, b_r1, b_ro = self.r1[jc], self.ro[jc], self.r1[jb], self.ro[jb]
            step = (j0 < nS) & ~(c_r1 > r)
            j = j0 + step
            ok &= j < nS
            g_r1, g_ro = np.where(step, c_r1, b_r1), np.where(step, c_ro, b_ro)
            ok &= ~((j > 0) & (r > g_r1) & (r < g_ro))
            shell = np.minimum(j, nS - 1)
            below0 = r < self.shell0_miss
            cand = (r > self.mirror_miss) if self.cand_on else np.zeros(r.shape, dtype=bool)
        self.both = bool(np.any(ok & below0 & cand))
        code = np.where(~ok, 0, np.where(below0, 1, np.where(cand, 3, 2)))
        return (code << 6 | shell).astype(np.uint32)

    def build(self):
        """(breakpoints, verdict words, cells) as build_radial_table makes them, or None where it gives up."""
        V = lambda x: int(self.by_compares(x)[0])
        cand = np.concatenate([self.r1, self.ro, [self.inner, self.ring_lo, self.ring_hi, self.r_last, self.mirror_miss, self.shell0_miss]])
        cand = np.unique(cand[np.isfinite(cand) & (cand > 0.0)])
        e, both = [], False
        for b in cand:
            v = (V(np.nextafter(b, -np.inf)), V(b), V(np.nextafter(b, np.inf)))
            both |= self.both
            if not (v[0] == v[1] == v[2]):
                e.append((float(b),) + v)
        far = V(np.finfo(np.float64).max)
        e.append((np.inf, far, far, far))
        for k, (b, lo, _, _) in enumerate(e):
            a = e[k - 1][0] if k else 0.0
            hi = b if np.isfinite(b) else 4.0 * (a + 1.0)
            if (e[k - 1][3] != lo) if k else (V(0.0) != lo or V(5e-324) != lo):
                return None
            pts = a + (hi - a) * (np.arange(1, 16) / 16.0)
            pts = pts[(pts > a) & (pts < hi)]
            if np.any(self.by_compares(pts) != lo):
                return None
        if both or len(e) > TABLE_MAX:
            return None
        bp = np.array([x[0] for x in e])
        words = np.array([x[1] | x[2] << 8 | x[3] << 16 for x in e], dtype=np.uint32)
        bcell = self.cell(bp)
        cells = np.empty(self.lut_n, dtype=np.uint8)
        for c in range(self.lut_n):
            k = int(np.searchsorted(bcell, c, side="left"))          # first breakpoint whose own cell is >= c
            several = int(np.sum(bcell == c)) > 1
            cells[c] = MARKED if (several or c == 0) else k
        return bp, words, cells

    def by_table(self, table, r):
        """The lookup of radial_verdict_table; the lanes of a marked cell evaluate the compares."""
        bp, words, cells = table
        r = np.atleast_1d(np.asarray(r, dtype=np.float64))
        k = cells[self.cell(r)].astype(np.int64)
        marked = k == MARKED
        kk = np.where(marked, 0, k)
        with np.errstate(invalid="ignore"):
            off = (r >= bp[kk]).astype(np.int64) + (r > bp[kk]).astype(np.int64)
        v = (words[kk] >> (8 * off).astype(np.uint32)) & np.uint32(0xFF)
        return np.where(marked, self.by_compares(r), v).astype(np.uint32), marked


def crafted_radii(geo, table, n_uniform, seed=1):
    """Every breakpoint moved by 0, +-1, +-2, +-8 ulp; every cell edge moved by 0, +-1 ulp; 0, the smallest denormal, 1e9, NaN;
    n_uniform uniform radii up to a little beyond the last shell."""
    def moved(x, ulps):
        out = [x]
        for u in ulps:
            for sign in (-np.inf, np.inf):
                y = x.copy()
                for _ in range(u):
                    y = np.nextafter(y, sign)
                out.append(y)
        return np.concatenate(out)
    bp = np.concatenate([geo.r1, geo.ro, [geo.inner, geo.ring_lo, geo.ring_hi]])
    for x in (geo.mirror_miss, geo.shell0_miss):
        if np.isfinite(x) and x > 0:
            bp = np.append(bp, x)
    if table is not None:
        bp = np.append(bp, table[0][np.isfinite(table[0])])
    edges = np.arange(geo.lut_n + 1) / geo.inv_step
    rng = np.random.default_rng(seed)
    return np.concatenate([moved(np.unique(bp), (1, 2, 8)), moved(edges, (1,)), [0.0, 5e-324, 1e9, np.nan],
                           rng.uniform(0.0, 1.05 * geo.r_last, n_uniform)])
