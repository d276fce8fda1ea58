"""The host boundary of every host-in encode: one double-buffered time-chunk pipeline.

``run_chunks`` moves a host tensor through the device in time chunks -- H2D of chunk i + 1 and D2H of chunk i - 1 on
their own streams while chunk i is encoded -- into a host result tensor (``SGPEncoder.encode_streamed``) or into a
host callback per chunk (``SGPEncoder.encode_to_shards``: shard files; ``multigpu``: the ranks' rows of the shared
result or their shard files).
"""
import threading

import torch


class RegisteredSink:
    """Destination of the pipelined host path: an ORDINARY (pageable) host tensor whose pages are
    registered with the HIP runtime block by block in a helper thread, so that the D2H copies go
    straight into it at PCIe speed -- no pinned bounce buffer, no host memcpy.  What remains is
    the kernel's first-touch cost of fresh pages (11-13 GB/s measured on the MI355X host,
    tools/probe_hostmem.py): the floor of ANY way of producing into new host memory.  The
    registration is dropped when the encode is done; the tensor is then plain memory again
    (the reference's drivers fork DataLoader workers that inherit it copy-on-write)."""
    BLOCK = 256 << 20

    def __init__(self, out):
        self.out = out
        self.rt = torch.cuda.cudart()
        page = 4096
        lo = out.data_ptr() // page * page
        hi = -(-(out.data_ptr() + out.numel() * out.element_size()) // page) * page
        self.base, self.blocks = out.data_ptr(), []
        self.todo = [(a, min(self.BLOCK, hi - a)) for a in range(lo, hi, self.BLOCK)]
        self.done_bytes = 0                     # bytes of ``out`` (from its start) that are registered
        self.failed = False
        self.cv = threading.Condition()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        for addr, size in self.todo:
            ok = False
            try:
                ok = int(self.rt.cudaHostRegister(addr, size, 0)) == 0
            except Exception:
                ok = False
            with self.cv:
                if ok:
                    self.blocks.append(addr)
                    self.done_bytes = addr + size - self.base
                else:
                    self.failed = True
                self.cv.notify_all()
            if not ok:
                return

    def wait(self, end_byte):
        """True once bytes [0, end_byte) of the tensor are registered; False if registration is
        not available (the caller then goes through its pinned slot)."""
        with self.cv:
            while self.done_bytes < end_byte and not self.failed:
                self.cv.wait()
            return self.done_bytes >= end_byte

    def pieces(self, b0, b1):
        """[b0, b1) (bytes from the tensor's start) cut at the block boundaries: one asynchronous
        copy must stay inside ONE registered range."""
        first = self.todo[0][0] - self.base                 # <= 0: start of block 0
        cuts = [b0]
        k = (b0 - first) // self.BLOCK + 1
        while first + k * self.BLOCK < b1:
            cuts.append(first + k * self.BLOCK)
            k += 1
        cuts.append(b1)
        return list(zip(cuts[:-1], cuts[1:]))

    def close(self):
        self.thread.join()
        for addr in self.blocks:
            try:
                self.rt.cudaHostUnregister(addr)
            except Exception:
                pass
        self.blocks = []


def run_chunks(x, T, tc, encode, dev, n_rows, d_out, *, rows=None, out=None, register=True, sink=None, events=None,
               store_dtype=None, overflow=None):
    """Host ``x[T, ...]`` -> ``encode(xs, oc)`` per time chunk of ``tc`` steps -> ``out`` or ``sink``.

    ``encode`` only enqueues on the current stream: it reads ``xs[n, n_rows, F]`` and writes ``oc[n, n_rows, d_out]``
    (device slots).  Input: ``x[t0:t0 + n]`` goes to the device straight from ``x`` when it is pinned float32 and
    ``rows`` is None, else through a pinned slot the host fills -- a copy (+ dtype cast), the rows ``x[:, rows]`` of a
    slice ``rows``, or an ``index_select`` of index ``rows``.  Output: into ``out`` (contiguous host ``[T, n_rows,
    d_out]``) straight from the device when it is pinned or, with ``register``, its pages are registered in time
    (``RegisteredSink``), else through a pinned bounce slot the host copies out; without ``out`` every chunk goes
    through a pinned slot to ``sink(t0, n, rows_tensor)``.  Two slots each way when there is more than one chunk: the
    H2D into a slot waits for the compute that last read it, the compute for its slot's H2D and for the D2H that last
    emptied its output slot, the host for the previous H2D of a pinned input slot before it refills it -- nothing on
    the compute stream waits for the host.  On return every chunk has reached ``out`` / ``sink``.  ``events``: a list
    that receives per chunk ``(compute start, compute end, d2h end)`` timing events.

    ``store_dtype`` (bfloat16 / float16): the chunk is still encoded into its fp32 device slot, then packed on the
    compute stream into a 16-bit device slot (``hip.pack_rows``; float16 counts its overflows into ``overflow``, a
    one-element int64 device tensor), and that slot is what leaves the device: ``out``, the pinned output slots and
    what ``sink`` receives are all in the store dtype -- half the D2H bytes."""
    if T == 0:
        return
    if store_dtype is not None:
        from . import hip
        hip.store_code(store_dtype)
        if out is not None and out.dtype != store_dtype:
            raise ValueError(f"out is {out.dtype}, store_dtype is {store_dtype}")
    out_dtype = torch.float32 if store_dtype is None else store_dtype
    esize = 4 if store_dtype is None else 2
    starts = list(range(0, T, tc))
    nbuf = 2 if len(starts) > 1 else 1
    timing = events is not None
    direct_in = rows is None and x.is_pinned() and x.dtype == torch.float32
    xin = [torch.empty(tc, n_rows, x.shape[2], dtype=torch.float32, device=dev) for _ in range(nbuf)]
    buf = [torch.empty(tc, n_rows, d_out, dtype=torch.float32, device=dev) for _ in range(nbuf)]
    # what the D2H reads: the fp32 slot itself, or its packed 16-bit copy
    wire = buf if store_dtype is None else [torch.empty(tc, n_rows, d_out, dtype=store_dtype, device=dev)
                                            for _ in range(nbuf)]
    pin_in = None if direct_in else [torch.empty(tc, n_rows, x.shape[2], dtype=torch.float32, pin_memory=True)
                                     for _ in range(nbuf)]
    # pinned output slots: every chunk passes one on its way to ``sink``; into ``out`` only a bounced chunk (allocated
    # when that first happens)
    pin_out = [torch.empty(tc, n_rows, d_out, dtype=out_dtype, pin_memory=True) if out is None else None
               for _ in range(nbuf)]
    out_pinned = out is not None and out.is_pinned()
    reg = RegisteredSink(out) if out is not None and register and not out_pinned else None
    main = torch.cuda.current_stream(dev)
    # high-priority copy streams: the runtime spreads streams of one priority over a few hardware queues, and a copy
    # stream that shares the compute stream's queue runs in its order -- the compute of chunk i + 1 then waits for the
    # D2H of chunk i.  High-priority streams get hardware queues of their own.
    h2d, d2h = torch.cuda.Stream(dev, priority=-1), torch.cuda.Stream(dev, priority=-1)
    ev_h2d = [None] * nbuf            # the input slot holds its chunk
    ev_done = [None] * nbuf           # compute of the slot's chunk finished
    ev_d2h = [None] * nbuf            # the chunk has left buf[slot] (wire[slot])
    bounced = [False] * nbuf          # the chunk sits in pin_out[slot], not in out
    row_bytes = n_rows * d_out * esize

    def stage_in(i):
        s, t0 = i % nbuf, starts[i]
        n = min(tc, T - t0)
        src = x[t0:t0 + n]
        if not direct_in:
            if ev_h2d[s] is not None:
                ev_h2d[s].synchronize()                          # the slot's previous H2D has read it
            if isinstance(rows, torch.Tensor):
                torch.index_select(src if src.dtype == torch.float32 else src.float(), 1, rows, out=pin_in[s][:n])
            else:
                pin_in[s][:n].copy_(src if rows is None else src[:, rows])     # host copy / gather (+ dtype cast)
            src = pin_in[s][:n]
        with torch.cuda.stream(h2d):
            if ev_done[s] is not None:
                h2d.wait_event(ev_done[s])                       # the chunk that used xin[s] is encoded
            xin[s][:n].copy_(src, non_blocking=True)
            ev_h2d[s] = torch.cuda.Event()
            ev_h2d[s].record(h2d)

    def send_out(i):
        """D2H of chunk i: straight into ``out`` when it is pinned or its pages are registered, else into a pinned
        slot that ``drain`` hands on."""
        s, t0 = i % nbuf, starts[i]
        n = min(tc, T - t0)
        direct = out_pinned or (reg is not None and reg.wait((t0 + n) * row_bytes))
        if not direct and pin_out[s] is None:
            pin_out[s] = torch.empty(tc, n_rows, d_out, dtype=out_dtype, pin_memory=True)
        bounced[s] = not direct
        with torch.cuda.stream(d2h):
            d2h.wait_event(ev_done[s])
            if direct:
                src, out_flat = wire[s][:n].reshape(-1), out.view(-1)
                e0 = t0 * (row_bytes // esize)
                cuts = [(t0 * row_bytes, (t0 + n) * row_bytes)] if out_pinned else \
                    reg.pieces(t0 * row_bytes, (t0 + n) * row_bytes)
                for a, b in cuts:
                    out_flat[a // esize:b // esize].copy_(src[a // esize - e0:b // esize - e0], non_blocking=True)
            else:
                pin_out[s][:n].copy_(wire[s][:n], non_blocking=True)
            ev_d2h[s] = torch.cuda.Event(enable_timing=timing)
            ev_d2h[s].record(d2h)

    def drain(i):
        s, t0 = i % nbuf, starts[i]
        n = min(tc, T - t0)
        if bounced[s]:
            ev_d2h[s].synchronize()                              # (the device is busy with the next chunk meanwhile)
            if out is None:
                sink(t0, n, pin_out[s][:n])
            else:
                out[t0:t0 + n].copy_(pin_out[s][:n])             # host memcpy into pageable memory
            bounced[s] = False

    try:
        stage_in(0)
        for i, t0 in enumerate(starts):
            s = i % nbuf
            n = min(tc, T - t0)
            if i + 1 < len(starts):
                stage_in(i + 1)
            main.wait_event(ev_h2d[s])
            if ev_d2h[s] is not None:
                drain(i - nbuf)                                  # chunk i - nbuf leaves pin_out[s] ...
                main.wait_event(ev_d2h[s])                       # ... and has left buf[s]
            if timing:
                c0 = torch.cuda.Event(enable_timing=True)
                c0.record(main)
            encode(xin[s][:n], buf[s][:n])
            if store_dtype is not None:
                hip.pack_rows(buf[s][:n], wire[s][:n], overflow=overflow)
            ev_done[s] = torch.cuda.Event(enable_timing=timing)
            ev_done[s].record(main)
            send_out(i)
            if timing:
                events.append((c0, ev_done[s], ev_d2h[s]))
        for i in range(max(0, len(starts) - nbuf), len(starts)):
            drain(i)
        d2h.synchronize()
        main.wait_stream(h2d)
        main.wait_stream(d2h)
    finally:
        if reg is not None:
            torch.cuda.synchronize(dev)
            reg.close()
