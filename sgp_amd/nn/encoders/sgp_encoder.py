import torch
from torch import nn

from ... import hip, hostpipe, tune
from ..reservoir import Reservoir
from ._args import add_reservoir_args, add_spatial_args
from .sgp_spatial_encoder import SGPSpatialEncoder


class SGPEncoder(nn.Module):
    """SGP's training-free spatiotemporal encoder, ``lib/nn/encoders/sgp_encoder.py:9-51``:
    reservoir over time, then K-hop graph-shift propagation over nodes.

    The device path allocates the final ``[T, N, D_out]`` tensor once; the reservoir
    writes its states straight into block 0, every hop reads one block and writes the next
    and the global-mean block is filled last -- the ``stack``/``rearrange``/``cat`` copies of
    the reference (reservoir.py:178-183, sgp_spatial_encoder.py:35) never happen.
    """

    def __init__(self,
                 input_size,
                 reservoir_size,
                 reservoir_layers,
                 leaking_rate,
                 spectral_radius,
                 density,
                 input_scaling,
                 receptive_field,
                 bidirectional,
                 alpha_decay,
                 global_attr,
                 add_self_loops=False,
                 undirected=False,
                 reservoir_activation='tanh'):
        super(SGPEncoder, self).__init__()
        self.reservoir = Reservoir(input_size=input_size,
                                   hidden_size=reservoir_size,
                                   input_scaling=input_scaling,
                                   num_layers=reservoir_layers,
                                   leaking_rate=leaking_rate,
                                   spectral_radius=spectral_radius,
                                   density=density,
                                   activation=reservoir_activation,
                                   alpha_decay=alpha_decay)
        self.sgp_encoder = SGPSpatialEncoder(
            receptive_field=receptive_field,
            bidirectional=bidirectional,
            undirected=undirected,
            add_self_loops=add_self_loops,
            global_attr=global_attr)
        self._side_streams = {}

    @property
    def output_size(self):
        return self.sgp_encoder.num_blocks() * self.reservoir.output_size

    # Small graphs: the reservoir is a serial chain of T steps on ceil(N / 16) CUs (PEMS-BAY: 21 of
    # 256) and the hops are bandwidth-bound on all of them.  Up to `overlap_tiles` node tiles, and when
    # the hops are worth it (their estimated time >= a tenth of the chain's), the time axis is cut
    # into up to `overlap_chunks` pieces and the hops (+ global mean) of piece i run on a second stream under
    # the reservoir of piece i + 1 (state carried on the device: bit-identical to one pass).
    # PEMS-BAY shape: 107 -> 93 ms per pass in round 2 (the chain runs ~13 % slower beside the hops -- the clock under
    # load, not its neighbours: its own compute units and no row wait changed nothing).
    # Round 5 (chain 0.76 us per step, hops 33 of the 39 ms beside it): 8 pieces 49.0 ms, 12: 45.2, 16: 45.0, 24: 48.3 -- the tail is the last piece's hops.
    overlap_tiles = 128
    overlap_chunks = 16
    overlap_chunks_time_parallel = 1   # time chunks of that pipeline when the reservoir runs as time pieces (SGP_TUNE=overlap_chunks_tp)
    overlap_masked_tiles = 32      # the chain gets its own compute units up to this many node tiles (hip.cu_masked_streams)

    def _overlap_pieces(self, T, N):
        if (N + 15) // 16 > self.overlap_tiles:
            return 1
        L, R = len(self.reservoir.reservoir_layers), self.reservoir.hidden_size
        chain_us = (0.27 + 3.0e-5 * R * R) * L                # per step: 0.39 us at R = 64, 0.76 at 128 (measured)
        hop_us = (self.sgp_encoder.num_blocks() - 1) * N * L * R * 8 / 4e6   # bytes of the hop blocks at ~4 TB/s
        share = hop_us / chain_us
        # hops as long as the chain (PEMS-BAY shape, 0.9): 16 pieces; a tenth of it (METR-LA shape, 0.14): 4 pieces take
        # 14.2 ms against 14.8 in one piece, 14.5 in 8 and 15.0 in 16 -- every piece costs a launch gap of the chain
        pieces = self.overlap_chunks if share >= 0.5 else 8 if share >= 0.25 else 4 if share >= 0.1 else 1
        pieces = tune.get("overlap_chunks", pieces, int)
        while pieces > 1 and T < 64 * pieces:                  # a sequence too short for the count takes the next smaller one
            pieces //= 2
        return max(1, pieces)

    def _state_bound(self, state=None):
        """Upper bound of |reservoir state| where one holds: a leaky average ``(1 - a) h + a act(.)`` of values in
        [-1, 1] stays in [-1, 1] (tanh; self_norm rows have unit 2-norm) PROVIDED every layer's leaking rate lies in
        [0, 1] (the reference accepts any float, reservoir.py:109-123) and the recurrence starts inside the
        interval -- from zero, or from a state this encoder produced itself under the same premises (marked
        ``_sgp_unit_bounded`` by ``encode_device``).  Everything else -- relu / identity, a leaking rate outside
        [0, 1], a state handed in by the caller -- returns None: the hop measures its operand."""
        if self.reservoir.mode not in ("tanh", "self_norm"):
            return None
        if not all(0.0 <= float(l.alpha) <= 1.0 for l in self.reservoir.reservoir_layers):
            return None
        if state is not None and not hip.is_unit_bounded(state):
            return None
        return 1.0

    def encode_device(self, x, ops, out=None, state=None, timeline=None):
        """x[T, N, F] CUDA float32 -> out[T, N, D_out] on the same device.  ``state`` [L, N, R]:
        reservoir state carried across calls (updated in place); ``timeline``: see
        ``sgp_preprocessing.propagate_into``."""
        T, N, _ = x.shape
        d_h = self.reservoir.output_size
        if out is None:
            out = torch.empty(T, N, self.output_size, dtype=torch.float32, device=x.device)
        chunks = self._overlap_pieces(T, N)
        time_parallel = chunks > 1 and self.reservoir.time_parallel(T, N, x.device)
        if time_parallel:
            # the reservoir runs as time pieces on the whole chip: few, long time chunks (the chain of chunk c + 1 under
            # the hops of chunk c), ordinary streams -- the chain is no longer a handful of workgroups to fence off
            chunks = max(1, min(tune.get("overlap_chunks_tp", self.overlap_chunks_time_parallel, int), chunks))
            while chunks > 1 and not self.reservoir.time_parallel(T // chunks, N, x.device):
                chunks //= 2
        x_bound = self._state_bound(state)
        # global_attr: the column sums of the states come from the reservoir kernel where it has them
        # in registers (fused stacked kernel); the other kernels keep the fused mean + broadcast pass
        want_sums = self.sgp_encoder.global_attr and self.reservoir.produces_col_sums(x)
        if chunks <= 1:
            sums = torch.empty(T, d_h, dtype=torch.float32, device=x.device) if want_sums else None
            self.reservoir.encode_into(x, out[:, :, :d_h], state, col_sums=sums)
            self.sgp_encoder.encode_into(out, d_h, ops, timeline, col_sums=sums, x_bound=x_bound)
            if state is not None and x_bound is not None:
                hip.mark_unit_bounded(state)                  # (carried on: encode_streamed, the time pieces below)
            return out
        if state is None:
            state = self.zero_state(N, x.device)
        main = torch.cuda.current_stream(x.device)
        key = str(x.device)
        if key not in self._side_streams:
            self._side_streams[key] = torch.cuda.Stream(device=x.device)
        side, chain = self._side_streams[key], main
        # The chain (one wave per SIMD on ceil(N / 16) CUs) and the hops (every CU) on DISJOINT compute units: the small
        # kernels between two pieces of the chain (weight packing) no longer queue behind hop workgroups (65 -> 5 us
        # each; PEMS-BAY shape 51.2 -> 48.6 ms per pass).  Up to 32 tiles.
        tiles = (N + 15) // 16
        if tiles <= self.overlap_masked_tiles and tune.get("overlap_cu_mask", 1, int) and not time_parallel:
            pair = hip.cu_masked_streams(x.device, (tiles + 7) // 8 * 8)
            if pair is not None:
                chain, side = pair
        side.wait_stream(main)                                  # (out / earlier work of the caller)
        if chain is not main:
            chain.wait_stream(main)
        for j in range(chunks):
            t0, t1 = T * j // chunks, T * (j + 1) // chunks
            with torch.cuda.stream(chain):
                sums = torch.empty(t1 - t0, d_h, dtype=torch.float32, device=x.device) if want_sums else None
                self.reservoir.encode_into(x[t0:t1], out[t0:t1, :, :d_h], state, col_sums=sums)
                ready = torch.cuda.Event()
                ready.record(chain)
            with torch.cuda.stream(side):
                side.wait_event(ready)
                self.sgp_encoder.encode_into(out[t0:t1], d_h, ops, timeline, col_sums=sums,
                                             x_bound=x_bound)
                if sums is not None:
                    sums.record_stream(side)
        main.wait_stream(side)
        if chain is not main:
            main.wait_stream(chain)
        return out

    # Device-memory budget for one pass (bytes); None = 80 % of what is free right now.  Host
    # inputs whose input + embedding exceed it are encoded in time chunks (see encode_streamed).
    max_device_bytes = None

    def _budget(self):
        if self.max_device_bytes is not None:
            return int(self.max_device_bytes)
        free, _ = torch.cuda.mem_get_info()
        return int(0.8 * free)

    # Host inputs larger than this many bytes (input + embedding) take the pipelined path even
    # when they would fit the device: PCIe then runs under the compute instead of after it.
    stream_threshold_bytes = 256 << 20
    stream_chunk_bytes = 1 << 30          # embedding bytes per time chunk of the pipelined path

    # ---- the 16-bit embedding store ----------------------------------------------------------------
    # The format the last encode of this encoder stored its product in (None: float32); describe() records it.
    store_dtype = None

    def _overflow_counter(self, store_dtype, dev):
        """The one device counter of an encode's float16 overflows (finite states that became infinite); bfloat16 has
        float32's exponent range and needs none."""
        return torch.zeros(1, dtype=torch.int64, device=dev) if store_dtype == torch.float16 else None

    @staticmethod
    def _raise_on_overflow(counter):
        """Read once, after the pipeline has drained."""
        lost = 0 if counter is None else int(counter.item())
        if lost:
            raise OverflowError(f"store_dtype=torch.float16: {lost} finite embedding values exceed float16's range "
                                f"(65504) and became infinite; store in torch.bfloat16, which has float32's range")

    def encode_device_packed(self, x, ops, out=None, store_dtype=torch.bfloat16, t_chunk=None, state=None):
        """x[T, N, F] CUDA float32 -> the embedding [T, N, D_out] in ``store_dtype`` (bfloat16 / float16) on the same
        device: ``t_chunk`` steps at a time are encoded into ONE float32 scratch (``encode_device``) and packed into the
        resident 16-bit tensor (``hip.pack_rows``, round-to-nearest-even: bit-equal to ``.to(store_dtype)`` of the
        float32 embedding).  HBM holds the 16-bit embedding plus one scratch chunk.  The reservoir state is carried
        across the chunks as ``encode_streamed`` carries it.  ``t_chunk`` defaults to ``stream_chunk_bytes`` of
        float32 embedding, at least 32 steps.  float16 raises ``OverflowError`` if a finite value became infinite."""
        hip.store_code(store_dtype)
        hip.require_gpu()
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3:
            raise ValueError("encode_device_packed takes a CUDA float32 tensor [T, N, F]")
        T, N, _ = x.shape
        D = self.output_size
        if out is None:
            out = torch.empty(T, N, D, dtype=store_dtype, device=x.device)
        elif (out.device != x.device or out.dtype != store_dtype or tuple(out.shape) != (T, N, D)
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {store_dtype} tensor of shape {(T, N, D)} on {x.device}")
        self.store_dtype = store_dtype
        if T == 0:
            return out
        if t_chunk is None:
            t_chunk = max(32, self.stream_chunk_bytes // max(1, N * D * 4))
        tc = max(1, min(int(t_chunk), T))
        if state is None:
            state = self.zero_state(N, x.device)
        if x.stride(2) != 1:
            x = x.contiguous()
        scratch = torch.empty(tc, N, D, dtype=torch.float32, device=x.device)
        lost = self._overflow_counter(store_dtype, x.device)
        for t0 in range(0, T, tc):
            n = min(tc, T - t0)
            self.encode_device(x[t0:t0 + n], ops, out=scratch[:n], state=state)
            hip.pack_rows(scratch[:n], out[t0:t0 + n], overflow=lost)
        self._raise_on_overflow(lost)
        return out

    def encode_streamed(self, x, ops, t_chunk, out=None, store_dtype=None):
        """Host tensor x[T, N, F] -> host tensor [T, N, D_out], ``t_chunk`` steps at a time,
        transfers overlapped with the compute (the drivers hand over host tensors,
        lib/utils.py:24-31): two device buffers per direction, H2D of chunk i+1 (through a pinned
        slot) and D2H of chunk i-1 on their own streams while chunk i is encoded; the D2H goes
        straight into the result tensor, whose pages a helper thread registers with the runtime
        ahead of the copies (``hostpipe.run_chunks`` / ``RegisteredSink``; pinned bounce slots + a host
        memcpy if the runtime refuses).  The recurrence is
        carried across chunks in a device-resident state ``[L, N, R]`` and the propagation is
        independent per time step, so the result is bit-identical to a single pass.  This is
        also how embeddings larger than the 288 GB of HBM (BASELINE config C5: 629 GB) or than
        the free memory are produced.  The returned tensor is ordinary (pageable) host memory:
        the reference's drivers fork DataLoader workers that inherit it copy-on-write.

        ``out``: a caller-supplied contiguous float32 host tensor ``[T, N, D_out]`` to fill instead
        of a fresh one.  A FRESH result tensor costs this host a page fault + zeroing per page
        (11-13 GB/s) -- more than the PCIe transfer; a tensor that is re-used between
        calls (or was touched before) skips that, and a pinned one (``.pin_memory()``) is written
        by the D2H copies directly, without the registration thread.

        ``store_dtype`` (bfloat16 / float16; or an ``out`` of that dtype): every chunk is packed on the device after
        its hops and leaves it in 16 bits -- half the D2H bytes and half the host tensor; the result is bit-equal to
        ``.to(store_dtype)`` of the float32 result.  float16 raises ``OverflowError`` if a finite value became
        infinite."""
        if store_dtype is None and out is not None and out.dtype in hip.STORE_CODES:
            store_dtype = out.dtype
        if store_dtype is not None:
            hip.store_code(store_dtype)
            if out is not None and out.dtype != store_dtype:
                raise ValueError(f"out is {out.dtype}, store_dtype is {store_dtype}")
        hip.require_gpu()
        T, N, _ = x.shape
        dev = torch.device("cuda", torch.cuda.current_device())
        D = self.output_size
        dtype = torch.float32 if store_dtype is None else store_dtype
        if out is None:
            out = torch.empty(T, N, D, dtype=dtype)
        elif (out.is_cuda or out.dtype != dtype or tuple(out.shape) != (T, N, D)
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {str(dtype)[6:]} host tensor of shape {(T, N, D)}")
        state = self.zero_state(N, dev)
        self.store_dtype = store_dtype
        lost = self._overflow_counter(store_dtype, dev)
        hostpipe.run_chunks(x, T, max(1, min(int(t_chunk), T)),
                            lambda xs, oc: self.encode_device(xs, ops, out=oc, state=state),
                            dev, N, D, out=out, register=self.register_output, store_dtype=store_dtype, overflow=lost)
        self._raise_on_overflow(lost)
        return out

    def encode_to_shards(self, x, ops, shard_dir, shard_steps, store_dtype=None):
        """Host tensor x[T, N, F] -> time shards on disk, ``shard_steps`` steps each, through the pipeline of
        ``encode_streamed``: embeddings larger than host RAM (configuration C5 is 629 GB,
        ``experiments/run_largescale_sgp.py:208-212``).  The host holds at most two pinned shard-sized slots (the
        pipeline's double buffer) plus the copy of the shard being written.  The reservoir state is carried on the
        device, the propagation is independent per step: the shards are bit-identical to slices of one pass.
        Returns a ``sgp_amd.datasets.ShardedEmbedding`` (``load_steps(t0, t1)`` reads any time range back).
        ``store_dtype`` (bfloat16 / float16): the shards hold the embedding in 16 bits, packed on the device."""
        import os
        from ...datasets.sharded import ShardedEmbedding
        if store_dtype is not None:
            hip.store_code(store_dtype)
        hip.require_gpu()
        T, N, F = x.shape
        os.makedirs(shard_dir, exist_ok=True)
        dev = torch.device("cuda", torch.cuda.current_device())
        D = self.output_size
        per_step = N * (F + D) * 4 + (0 if store_dtype is None else N * D * 2)     # (+ the 16-bit slot beside the fp32 one)
        ts = max(1, min(int(shard_steps), T, self._budget() // max(1, 2 * per_step)))    # two slots each way
        state = self.zero_state(N, dev)
        self.store_dtype = store_dtype
        lost = self._overflow_counter(store_dtype, dev)
        paths = []

        def sink(t0, n, emb):
            paths.append(os.path.join(shard_dir, f"embedding_t{t0:08d}.pt"))
            ShardedEmbedding.write_shard(paths[-1], t0, n, None, emb)

        hostpipe.run_chunks(x, T, ts, lambda xs, oc: self.encode_device(xs, ops, out=oc, state=state),
                            dev, N, D, sink=sink, store_dtype=store_dtype, overflow=lost)
        self._raise_on_overflow(lost)
        dtype = torch.float32 if store_dtype is None else store_dtype
        ShardedEmbedding.write_index(shard_dir, paths, (T, N, D), dtype=dtype)
        return ShardedEmbedding(paths, T, N, D, dtype=dtype)

    def zero_state(self, n_nodes, device):
        """Reservoir state ``[L, n_nodes, R]`` carried across time chunks: zero, hence marked unit-bounded
        (see ``_state_bound``)."""
        state = torch.zeros(len(self.reservoir.reservoir_layers), n_nodes, self.reservoir.hidden_size,
                            dtype=torch.float32, device=device)
        hip.mark_unit_bounded(state)
        return state

    # D2H straight into the (registered) result tensor; False = pinned bounce slots + host memcpy
    register_output = True

    def forward(self, x, edge_index, edge_weight, return_device=False, out=None, gpus=None, shard_dir=None,
                shard_steps=None, store_dtype=None, t_chunk=None):
        # x : [t n f]; ``return_device=True`` keeps the embedding of a host input on the GPU
        # (the next row f1 consumes it there: sgp_amd.datasets.IIDDataset); ``out``: host tensor
        # [t, n, d_out] to fill (host inputs only; see encode_streamed); ``gpus``: number of GPUs the
        # graph is node-partitioned over (None: SGP_AMD_GPUS, default 1; 0 / "all": every visible GPU) --
        # the call stays a single-process call on a host tensor, the ranks are started and joined inside
        # (sgp_amd/multigpu.py)
        # ``shard_dir``: write the embedding as shard files instead of returning one host tensor (embeddings
        # larger than host RAM) -- time shards of ``shard_steps`` steps on one GPU, time x node-block shards of
        # the ranks with ``gpus`` > 1; the call then returns a ``sgp_amd.datasets.ShardedEmbedding``
        # ``store_dtype`` (torch.bfloat16 / torch.float16, or an ``out`` of that dtype): the embedding is stored in 16
        # bits -- host tensor, shards or, with ``return_device`` / a device input, the resident tensor
        # (encode_device_packed, ``t_chunk`` steps per scratch chunk); one GPU only
        from ... import multigpu
        n_gpus = multigpu.resolve_gpus(gpus)
        if store_dtype is None and out is not None and out.dtype in hip.STORE_CODES:
            store_dtype = out.dtype
        if store_dtype is not None:
            hip.store_code(store_dtype)
            if n_gpus > 1:
                raise ValueError("store_dtype is a single-GPU path: the ranks of gpus > 1 exchange and write float32")
            return self._forward_stored(x, edge_index, edge_weight, return_device, out, shard_dir, shard_steps,
                                        store_dtype, t_chunk)
        self.store_dtype = None
        if n_gpus > 1:
            if x.is_cuda or return_device:
                raise ValueError("gpus > 1 takes a host tensor and returns a host tensor in the original node "
                                 "order (device shards live in the rank processes)")
            if shard_dir is not None:
                from ...datasets.sharded import ShardedEmbedding
                paths = multigpu.encode_multi_gpu(self, x, edge_index, edge_weight, n_gpus, shard_dir=shard_dir)
                shape = (x.shape[0], x.shape[1], self.output_size)
                ShardedEmbedding.write_index(shard_dir, paths, shape)
                return ShardedEmbedding(paths, *shape)
            return multigpu.encode_multi_gpu(self, x, edge_index, edge_weight, n_gpus, out=out)
        if shard_dir is not None:
            if x.is_cuda or return_device or out is not None:
                raise ValueError("shard_dir takes a host tensor and writes shard files")
            ops = self.sgp_encoder.operators(x.size(-2), edge_index, edge_weight)
            return self.encode_to_shards(x, ops, shard_dir, shard_steps or 256)
        dev = x.device
        ops = self.sgp_encoder.operators(x.size(-2), edge_index, edge_weight)
        xg = x.float()
        if not xg.is_cuda:
            hip.require_gpu()
            T, N, F = xg.shape
            per_step = N * (F + self.output_size) * 4
            budget = self._budget()
            if return_device:
                if T * per_step > budget:
                    raise RuntimeError("return_device=True: the embedding does not fit the device")
                return self.encode_device(xg.cuda(), ops)
            if T * per_step > min(budget, self.stream_threshold_bytes) and T > 1:
                # two input + two output buffers on the device; chunks of >= 32 steps keep the
                # propagation kernels at their full-size rates
                t_chunk = max(1, min(budget // (2 * per_step),
                                     max(32, self.stream_chunk_bytes // max(1, N * self.output_size * 4))))
                return self.encode_streamed(xg, ops, t_chunk, out=out)
            if out is not None:
                return self.encode_streamed(xg, ops, T, out=out)
            xg = xg.cuda()
        if out is not None:
            raise ValueError("out= is for host inputs (a device input returns a device tensor)")
        if xg.stride(2) != 1:
            xg = xg.contiguous()
        return self.encode_device(xg, ops).to(dev)

    def _forward_stored(self, x, edge_index, edge_weight, return_device, out, shard_dir, shard_steps, store_dtype,
                        t_chunk):
        """``forward`` with ``store_dtype``: the same routes, every one through the pack kernel."""
        ops = self.sgp_encoder.operators(x.size(-2), edge_index, edge_weight)
        if shard_dir is not None:
            if x.is_cuda or return_device or out is not None:
                raise ValueError("shard_dir takes a host tensor and writes shard files")
            return self.encode_to_shards(x, ops, shard_dir, shard_steps or 256, store_dtype=store_dtype)
        xg = x.float()
        T, N, F = xg.shape
        D = self.output_size
        if xg.is_cuda or return_device:
            if out is not None:
                raise ValueError("out= is for host inputs (a device input returns a device tensor)")
            if t_chunk is None:
                t_chunk = max(32, self.stream_chunk_bytes // max(1, N * D * 4))
            t_chunk = max(1, min(int(t_chunk), max(1, T)))
            if not xg.is_cuda:
                hip.require_gpu()
                # the input, the 16-bit embedding and the one float32 scratch chunk
                if T * N * (F * 4 + D * 2) + t_chunk * N * D * 4 > self._budget():
                    raise RuntimeError("return_device=True: the embedding does not fit the device")
                xg = xg.cuda()
            return self.encode_device_packed(xg, ops, store_dtype=store_dtype, t_chunk=t_chunk)
        hip.require_gpu()
        # two input, two float32 and two 16-bit output slots on the device
        per_step = N * (F + D) * 4 + N * D * 2
        if t_chunk is None:
            t_chunk = T
            if T * per_step > min(self._budget(), self.stream_threshold_bytes) and T > 1:
                t_chunk = max(32, self.stream_chunk_bytes // max(1, N * D * 4))
        t_chunk = max(1, min(int(t_chunk), self._budget() // max(1, 2 * per_step)))
        return self.encode_streamed(xg, ops, t_chunk, out=out, store_dtype=store_dtype)

    def describe(self):
        """What makes an embedding re-derivable: constructor arguments, the
        per-layer leaking rates and every weight tensor."""
        res = self.reservoir
        sp = self.sgp_encoder
        return dict(
            encoder="SGPEncoder",
            kwargs=dict(input_size=res.input_size, reservoir_size=res.hidden_size,
                        reservoir_layers=res.num_layers, leaking_rate=res.leaking_rate,
                        spectral_radius=res.spectral_radius, density=res.density,
                        input_scaling=res.input_scaling, receptive_field=sp.receptive_field,
                        bidirectional=sp.bidirectional, alpha_decay=res.alpha_decay,
                        global_attr=sp.global_attr, add_self_loops=sp.add_self_loops,
                        undirected=sp.undirected, reservoir_activation=res.mode),
            alphas=[float(l.alpha) for l in res.reservoir_layers],
            # the format the last encode stored the embedding in ("bfloat16" / "float16"; None: float32)
            store_dtype=None if self.store_dtype is None else str(self.store_dtype)[6:],
            state_dict={k: v.detach().cpu().clone() for k, v in self.state_dict().items()})

    @staticmethod
    def add_model_specific_args(parser):
        add_reservoir_args(parser)
        add_spatial_args(parser)
        return parser
