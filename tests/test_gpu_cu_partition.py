"""The CU partition and the forward-FFT stream of the fold-bound geometries (planner.h plan_cu_partition) change where kernels run, not
what they compute: the laboratory library with both switched on against the product library, which has neither."""
import numpy as np
import pytest

import hfdl_synth as synth
from dumphfdl_amd import frontend as F

pytestmark = pytest.mark.gpu


def test_partition_and_fft_stream_change_nothing(gpu, monkeypatch):
    """2.4 Msps x 130 channels, the smallest fold-bound geometry of the suite: 20 blocks (a 16-block half closed by filling and four more
    closed by the poll), a draining poll, a ragged half of 5 blocks, a draining poll.  Channelizer output of three channels as uint32,
    every PDU field and every channel statistic are identical."""
    fs, cf, nch = 2_400_000, 10_000_000, 130
    rng = np.random.default_rng(9)
    freqs = [int(cf + (i - nch // 2) * 15_000 + 4_000) for i in range(nch)]
    bursts = [dict(freq=freqs[c], mode=int(rng.integers(0, 4)), octets=b"", t0=float(rng.uniform(0.1, 0.6)), amp=0.03, cfo=float(rng.uniform(-10, 10)))
              for c in (0, 64, 77, 129)]
    for b in bursts:
        b["octets"] = synth.make_pdu(rng, b["mode"])
    probe = gpu.Frontend(fs, cf, freqs[:1])
    n = probe.input_size
    probe.close()
    x = synth.synth_wideband(fs, cf, 25 * n, bursts, noise_sigma=0.012, seed=9)

    def run(partitioned):
        monkeypatch.setenv("HFDL_GPU_CU_PARTITION", "1")               # the product library does not read it
        fe = gpu.Frontend(fs, cf, freqs, lib=F.load_lab() if partitioned else None)
        monkeypatch.delenv("HFDL_GPU_CU_PARTITION")
        if partitioned:                    # a runtime that refuses CU masks gets plain streams and the text says so: then nothing was compared
            assert b"CU-masked streams refused" not in F.load_lab().hfdl_gpu_last_error()
        got, outs = [], []
        for b in range(25):
            fe.push_block(x[b * n:(b + 1) * n])
            if b in (19, 24):
                got += fe.poll_pdus()
                outs += [fe.read_tap(F.TAP_CHAN_OUT, c).view(np.uint32).copy() for c in (0, 64, 129)]
        stats = fe.all_channel_stats()
        fe.close()
        return sorted(got, key=lambda p: (p["freq"], p["sample_index"])), outs, stats

    ref, ref_outs, ref_stats = run(False)
    got, outs, stats = run(True)
    assert len(ref) >= 3 and got == ref and stats == ref_stats
    assert len(outs) == 6 and all(len(a) and np.array_equal(a, b) for a, b in zip(outs, ref_outs))
