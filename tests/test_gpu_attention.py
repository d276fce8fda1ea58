"""The attention kernels alone, through ``hip.attention_fwd`` / ``hip.attention_bwd``, against fp64: every case of
``tests/attention_forms.py`` forward and backward, with the operands as column ranges of one padded buffer in both
token layouts.  Criterion: ``allclose(rtol=1e-5, atol=1e-5 * max|ref|)`` and rel-Frobenius ``<= 1e-5`` for
every output and gradient; the CPU's own fp32 evaluation has to pass it first."""
import functools

import pytest
import torch

import attention_forms as AF
import transformer_ref as R
from sgp_amd import hip

pytestmark = pytest.mark.gpu
PAD = 4                # columns in front of and behind the operands: 16 bytes, so the ranges stay aligned
SENTINEL = -77.25


def passes(got, ref):
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    e = R.errors(got, ref)
    scale = float(ref.abs().max())
    return got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-5, atol=1e-5 * scale) and e[1] <= 1e-5, e


def check(got, ref, what, cpu32):
    ok32, e_cpu = passes(cpu32, ref)
    assert ok32, (what, "the CPU fp32 evaluation misses the criterion: choose another seed", e_cpu)
    ok, e = passes(got, ref)
    print(f"{what}: e_gpu {e[0]:.2e} / {e[1]:.2e}   e_cpu {e_cpu[0]:.2e} / {e_cpu[1]:.2e}")
    assert ok, (what, e)


def token_map(c, steps_batch_major=None):
    """``(TokenMap, row index [n_seq, L])`` of a case: ``'nodes'`` keeps a sequence's tokens contiguous; ``'steps'`` is
    time-major ``[L, M]`` rows, or for 65 sequences the batch-major ``[5, L, 13]`` rows of a ``[b, s, n]`` window."""
    q = torch.arange(c.n_seq)[:, None]
    t = torch.arange(c.L)[None, :]
    if c.layout == "nodes":
        tm = hip.TokenMap(1, c.L, 0, 1)
    elif c.n_seq == 65:
        tm = hip.TokenMap(13, c.L * 13, 1, 13)
    else:
        tm = hip.TokenMap(c.n_seq, 0, 1, c.n_seq)
    inner, outer, inr, tok = tm
    return tm, (q // inner) * outer + (q % inner) * inr + t * tok


@functools.lru_cache(maxsize=None)
def operands(c, seed=0, q_scale=1.0, same_keys=False):
    """Inputs of a case and its fp64 / CPU fp32 results, computed once: ``buf [rows, 3 E + 8]`` (q | k | v between
    padding columns), ``dout [rows, E]``, and per precision ``(o, dq, dk, dv)`` as ``[n_seq, L, E]``."""
    g = torch.Generator().manual_seed(1000 + seed)
    E = c.heads * c.d
    rows = c.n_seq * c.L
    buf = torch.randn(rows, 3 * E + 2 * PAD, generator=g)
    buf[:, PAD:PAD + E] *= q_scale
    tm, idx = token_map(c)
    if same_keys:                                                     # sequence 0: every key the same row
        buf[idx[0], PAD + E:PAD + 2 * E] = buf[idx[0, 0], PAD + E:PAD + 2 * E]
    dout = torch.randn(rows, E, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        q, k, v = (buf[idx][..., PAD + i * E:PAD + (i + 1) * E].to(dt).clone().requires_grad_(True) for i in range(3))
        o = R.attention(q, k, v, c.heads, bool(c.causal), c.q_first)
        o.backward(dout[idx][:, c.q_first:].to(dt))
        res[dt] = (o.detach(), q.grad, k.grad, v.grad)
    return buf, dout, tm, idx, res


def run_gpu(c, buf, dout, tm, backward=True):
    E = c.heads * c.d
    b = buf.cuda()
    q, k, v = (b[:, PAD + i * E:PAD + (i + 1) * E] for i in range(3))
    obuf = torch.full((b.shape[0], E + 2 * PAD), SENTINEL, device="cuda")
    out = obuf[:, PAD:PAD + E]
    lse = torch.empty(c.n_seq, c.heads, c.L, device="cuda")
    hip.attention_fwd(q, k, v, out, c.L, c.d, c.heads, c.n_seq, tm, c.causal, c.q_first, lse)
    if not backward:
        return obuf, lse, None
    dbuf = torch.full_like(b, SENTINEL)
    dq, dk, dv = (dbuf[:, PAD + i * E:PAD + (i + 1) * E] for i in range(3))
    hip.attention_bwd(dout.cuda(), q, k, v, out, lse, dq, dk, dv, c.L, c.d, c.heads, c.n_seq, tm, c.causal, c.q_first)
    return obuf, lse, dbuf


def judge(c, buf, dout, tm, idx, res, what):
    E = c.heads * c.d
    obuf, lse, dbuf = run_gpu(c, buf, dout, tm)
    o = obuf.cpu()
    assert (o[:, :PAD] == SENTINEL).all() and (o[:, PAD + E:] == SENTINEL).all(), "O: padding columns written"
    og = o[:, PAD:PAD + E][idx]                                       # [n_seq, L, E]
    assert (og[:, :c.q_first] == SENTINEL).all(), "O: rows below q_first written"
    r64, r32 = res[torch.float64], res[torch.float32]
    check(og[:, c.q_first:], r64[0], f"{what} O", r32[0])
    assert torch.isfinite(lse.reshape(c.n_seq, c.heads, c.L)[:, :, c.q_first:]).all()
    d = dbuf.cpu()
    assert (d[:, :PAD] == SENTINEL).all() and (d[:, PAD + 3 * E:] == SENTINEL).all(), "dQKV: padding columns written"
    for i, name in enumerate(("dQ", "dK", "dV")):
        got = d[:, PAD + i * E:PAD + (i + 1) * E][idx]
        if c.L == 1 and i < 2:
            # One key: P = 1 and dS = P (dP - delta) = dO.V - dO.O is zero in exact arithmetic, so dQ = dK = 0 and the
            # criterion has no scale to be relative to.  What fp32 returns is the rounding of the two sums that cancel;
            # the bound is the criterion's 1e-5 on the size of those sums times the other factor of the product.
            q, k, v = (buf[idx][..., PAD + j * E:PAD + (j + 1) * E].double() for j in range(3))
            terms = float((dout[idx].double().abs() * v.abs()).reshape(c.n_seq, c.heads, c.d).sum(-1).max())
            bound = 1e-5 * terms * float((k if i == 0 else q).abs().max()) / c.d ** 0.5
            assert float(r64[1 + i].abs().max()) == 0.
            print(f"{what} {name}: zero in exact arithmetic; gpu {float(got.abs().max()):.2e}, bound {bound:.2e}")
            assert float(got.abs().max()) <= bound
            continue
        check(got, r64[1 + i], f"{what} {name}", r32[1 + i])
    assert (d[:, PAD:PAD + E][idx][:, :c.q_first] == 0).all(), "dQ: rows below q_first are zeros"
    return obuf, dbuf


@pytest.mark.parametrize("c", AF.CASES, ids=lambda c: c.id)
def test_case_against_fp64(c):
    buf, dout, tm, idx, res = operands(c)
    o1, d1 = judge(c, buf, dout, tm, idx, res, c.id)
    o2, _, d2 = run_gpu(c, buf, dout, tm)
    assert torch.equal(o1, o2) and torch.equal(d1, d2), "not bit-identical from run to run"


BATCH_CASES = [c for c in AF.CASES if c.n_seq == 3 and c.L <= 130]


@pytest.mark.parametrize("c", BATCH_CASES, ids=lambda c: c.id)
def test_sequence_alone_and_permuted(c):
    """A sequence computed alone has the bits it has in the batch; permuting the sequences permutes the bits."""
    buf, dout, tm, idx, _ = operands(c)
    E = c.heads * c.d
    obuf, _, dbuf = run_gpu(c, buf, dout, tm)
    ob, db = obuf.cpu(), dbuf.cpu()
    one = c._replace(n_seq=1)
    tm1, idx1 = token_map(one)
    for s in range(3):
        o1, _, d1 = run_gpu(one, buf[idx[s]].contiguous(), dout[idx[s]].contiguous(), tm1)
        assert torch.equal(o1.cpu()[idx1[0]][c.q_first:, PAD:PAD + E], ob[idx[s]][c.q_first:, PAD:PAD + E]), s
        assert torch.equal(d1.cpu()[idx1[0]][:, PAD:PAD + 3 * E], db[idx[s]][:, PAD:PAD + 3 * E]), s
    perm = [2, 0, 1]
    pbuf, pdout = buf.clone(), dout.clone()
    for s in range(3):
        pbuf[idx[s]], pdout[idx[s]] = buf[idx[perm[s]]], dout[idx[perm[s]]]
    op, _, dp = run_gpu(c, pbuf, pdout, tm)
    for s in range(3):
        assert torch.equal(op.cpu()[idx[s]][c.q_first:], ob[idx[perm[s]]][c.q_first:])
        assert torch.equal(dp.cpu()[idx[s]], db[idx[perm[s]]])


def test_large_logits():
    """Scores near 80 before the softmax: finite, and within the criterion like every other case."""
    c = AF.Case(33, 32, 3, 3, 0, False, "nodes")
    buf, dout, tm, idx, res = operands(c, seed=3, q_scale=16.0)
    E = c.heads * c.d
    q, k = (buf[idx][..., PAD + i * E:PAD + (i + 1) * E].double().reshape(3, 33, 3, 32).transpose(1, 2) for i in range(2))
    top = float((q @ k.transpose(-1, -2)).abs().max() / 32 ** 0.5)
    print(f"largest |score| {top:.1f}")
    assert 60 <= top <= 100
    obuf, dbuf = judge(c, buf, dout, tm, idx, res, "large logits")
    assert torch.isfinite(obuf).all() and torch.isfinite(dbuf).all()


@pytest.mark.parametrize("causal", [0, 1])
def test_identical_logits(causal):
    """A sequence whose keys are all the same row: every visible key of a query has the same score."""
    c = AF.Case(33, 24, 3, 3, causal, False, "steps")
    buf, dout, tm, idx, res = operands(c, seed=5, same_keys=True)
    judge(c, buf, dout, tm, idx, res, f"identical logits causal {causal}")


def test_operand_checks_before_a_launch():
    x = torch.zeros(24, 40, device="cuda")
    tm = hip.TokenMap(1, 12, 0, 1)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        hip.attention_fwd(x[:, :12], x[:, 12:24], x[:, 24:36], torch.zeros(24, 12, device="cuda"), 12, 12, 1, 2, tm)
    with pytest.raises(ValueError, match="rows"):
        hip.attention_fwd(x[:, :8], x[:, 8:16], x[:, 16:24], torch.zeros(24, 8, device="cuda"), 12, 8, 1, 3, tm)
    with pytest.raises(RuntimeError, match="aligned"):                # a column range that starts on an odd float
        hip.attention_fwd(x[:, 1:9], x[:, 8:16], x[:, 16:24], torch.zeros(24, 8, device="cuda"), 12, 8, 1, 2, tm)
