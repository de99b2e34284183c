"""The two breakdowns of the histogram trace back to back on ONE context (MI355X box).

sart_trace_histogram_shells_device and sart_trace_histogram_channels_device go through one host path and one kernel body, and on a
context they share the placement of the LDS image tile (each narrows it for its own table), the scalar partials and the grid caches.
Demanded here, in SART_ACCUM_FIXED64: a shells launch, a channels launch, a shells launch and a plain histogram launch on one context
give the same raw int64 accumulator, slot for slot, and each block is the block a fresh context gives for that launch alone."""
import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L

from tests import test_gpu_channels as TC

pytestmark = pytest.mark.gpu

N_RAYS, SEED, OFFSET = 400_000, 7, 13
T = 3


def indicator_rates():
    """T indicator channels: the bands of the radius index (every fraction 0 or 1)."""
    total = TC.total_table()
    n_r = total.shape[0]
    band = np.minimum(np.arange(n_r) * T // n_r, T - 1)
    return np.stack([total * (band == t)[:, None] for t in range(T)]), total


def launch(rt, torch, kind, spectra, image_n):
    """Raw accumulator and block (None: the plain histogram) of one launch of `kind` into zeroed buffers."""
    p = TC.params(rt, N_RAYS, SEED, OFFSET, spectra, image_n, accumulate=True)
    acc = TC.zeros(torch, TC.acc_len(rt, p), torch.int64)
    blk = None
    if kind == "shells":
        blk = TC.zeros(torch, rt.shell_block_len(spectra), torch.int64)
        rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr())
    elif kind == "channels":
        blk = TC.zeros(torch, rt.channel_block_len(spectra, image_n), torch.int64)
        rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr())
    else:
        rt.trace_histogram_device(p, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy(), None if blk is None else blk.cpu().numpy()


def tracer(full):
    t = TC.Tracer(full)
    t.rt.set_source_channels(*indicator_rates())
    t.rt.set_accumulation_mode("fixed64")
    return t


@pytest.mark.parametrize("name", ["babyiaxo_xmm_rot", "cast_llnl"])
def test_breakdowns_back_to_back_on_one_context(name):
    import torch
    full = TC.setup_of(name)
    order = ("shells", "channels", "shells", "plain")
    with tracer(full) as rt:
        for spectra, image_n in ((True, 256), (False, 0)):
            got = [launch(rt, torch, kind, spectra, image_n) for kind in order]
            plain = got[3][0]
            assert plain[image_n * image_n + L.ACC["N_PASSED"]] > 100
            alone = {}
            for kind in ("shells", "channels"):
                with tracer(full) as fresh:
                    alone[kind] = launch(fresh, torch, kind, spectra, image_n)
                np.testing.assert_array_equal(alone[kind][0], plain)
            for kind, (acc, blk) in zip(order, got):
                np.testing.assert_array_equal(acc, plain, err_msg=kind)
                if blk is not None:
                    np.testing.assert_array_equal(blk, alone[kind][1], err_msg=kind)
            assert np.any(alone["shells"][1] != 0) and np.any(alone["channels"][1] != 0)
