"""The host time-chunk pipeline (``sgp_amd/hostpipe.py``) that every host-in encode runs: ``encode_streamed`` into a
host tensor, ``encode_to_shards`` and the ranks of ``multigpu`` into a per-chunk sink."""
import time

import pytest
import torch

from sgp_amd import hostpipe


@pytest.mark.gpu
@pytest.mark.parametrize("dest", ["sink", "pinned", "registered", "bounce"])
def test_pipeline_overlaps_transfers_with_the_next_chunk(dest):
    """Every destination: the D2H of chunk i runs while the device already encodes chunk i + 1 (event times), the host
    copies (gather, bounce, scatter) never sit between two chunks' compute, and the data arrive intact.  ``sink``: a
    rank's index gather into a per-chunk callback; ``pinned``: D2H straight into a pinned ``out``; ``registered``:
    straight into a pageable ``out`` whose pages a helper thread registers; ``bounce``: a pageable ``out`` through
    pinned slots."""
    dev = torch.device("cuda", 0)
    T, tc, n_own, f_in, d_out = 48, 8, 4000, 16, 1024
    x = torch.randn(T, 2 * n_own, f_in)
    rows = torch.arange(0, 2 * n_own, 2)
    want = x[:, rows].repeat(1, 1, d_out // f_in)
    got = torch.zeros(T, n_own, d_out)
    if dest == "sink":
        def sink(t0, n, emb):
            got[t0:t0 + n] = emb

        kw = dict(rows=rows, sink=sink)
    else:
        x = x[:, rows].contiguous()                                 # encode_streamed: the rows of x are the rows of out
        got = got.pin_memory() if dest == "pinned" else got
        kw = dict(out=got, register=dest == "registered")

    def encode(xs, oc):                                            # ~15 ms of device work per chunk, only enqueued
        torch.cuda._sleep(30_000_000)
        oc.copy_(xs.repeat(1, 1, d_out // f_in))

    hostpipe.run_chunks(x, T, tc, encode, dev, n_own, d_out, **kw)     # warm-up: slots from the caching allocators
    got.zero_()
    events = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hostpipe.run_chunks(x, T, tc, encode, dev, n_own, d_out, events=events, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert torch.equal(got, want)
    comp = [a.elapsed_time(b) for a, b, _ in events]
    d2h_after_next_start = [events[i + 1][0].elapsed_time(events[i][2]) for i in range(len(events) - 1)]
    gaps = [events[i][1].elapsed_time(events[i + 1][0]) for i in range(len(events) - 1)]
    print(f"{dest}: compute {[round(c, 2) for c in comp]} ms, gaps {[round(g, 3) for g in gaps]} ms, "
          f"wall {wall * 1e3:.1f} ms")
    assert min(d2h_after_next_start) > 0, d2h_after_next_start      # chunk i leaves while chunk i + 1 is being encoded
    assert max(gaps[1:]) < 0.5 * min(comp), (gaps, comp)            # nothing (host copies, D2H) between two chunks' compute
    assert wall * 1e3 < sum(comp) + 3 * max(comp), (wall, comp)
