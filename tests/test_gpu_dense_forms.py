"""One numerical case per launch form and epilogue of the dense decoder kernels (tests/dense_forms.py; the host half,
tests/test_dense_forms.py, shows that every case reaches the forms it names), through the BINDINGS ``hip.dense``,
``hip.dense_wgrad``, ``hip.row_segsum``, ``hip.masked_loss`` / ``_bwd`` (kind mae) and ``hip.grouped_linear`` / ``_dact`` / ``_transpose``
/ ``_wgrad``.

Every operand and every output a caller can hand over is a view with its row padding inside a buffer with GUARD floats
on either side; outputs, guards and padding hold a NaN bit pattern before the launch.  After it every float outside the
logical output is bitwise what it was, and no logical output element is NaN unless the reference is.

Reference: the same operation in fp64 on the CPU from the fp32 inputs (dense_forms.py; no call into sgp_amd).
* dropout masks are exact: the zeroed positions are those of the numpy Philox;
* linear and relu epilogues, every weight gradient and row_segsum: per element |got - ref64| <= (k_c + 3) 2^-23 S with
  k_c the contraction length and S the same expression on absolute values -- the standard bound of an fp32 sum of k_c
  products plus bias, keep scale and add (k_c + 3 roundings of 2^-24), with a factor 2; derived, not measured;
* silu and its derivative (``__expf`` and the hardware reciprocal): the criterion of
  test_gpu_sgp_model.test_dense_kernels_at_training_sizes_against_fp64, rtol 1e-5 and atol 1e-5 x the largest reference
  magnitude, which CPU fp32 torch of the same pre-activation has to pass first;
* masked_mae: the loss within 1e-6 relative of the fp64 value, the count exact.

After a device error (an exception out of the library or the runtime, as opposed to a failed comparison) every later case
fails without launching; nothing is retried."""
import os
import sys

import numpy as np
import pytest
import torch

from sgp_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_forms as DF                                                # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4                   # floats in front of and behind every buffer (16 bytes: keeps the alignment)
NAN_BITS = 0x7FC0BEEF       # a quiet NaN no arithmetic produces
_device_error = []


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    hip.require_gpu()


def guarded(rows, width, pad=0, off=0, data=None):
    """(whole buffer, view [rows, width]): rows ``width + pad`` floats apart, the first element ``off`` floats past a
    16-byte boundary, GUARD floats on either side; everything is NAN_BITS but the view, which holds ``data`` if given."""
    size = rows * (width + pad)
    buf = torch.full((GUARD + off + size + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + off:GUARD + off + size].view(rows, width + pad)[:, :width]
    if data is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(data)).reshape(rows, width))
    return buf, view


def outside(buf, base, view):
    """The bits of ``buf`` (``base`` or a copy of it) with the elements of ``view`` (a view into ``base``) zeroed."""
    bits = buf.clone()
    if view.numel():
        torch.as_strided(bits, view.shape, view.stride(), (view.data_ptr() - base.data_ptr()) // 4).zero_()
    return bits.view(torch.int32)


def launch(fn, *args, **kw):
    assert not _device_error, f"not launched: an earlier case ended in a device error: {_device_error[0]}"
    try:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out
    except Exception as e:
        _device_error.append(repr(e))
        raise


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def np64(t):
    return t.detach().cpu().double().numpy()


def check_bound(got, ref, S, k_c, what, family):
    """|got - ref| <= (k_c + 3) 2^-23 S per element; NaN only where the reference has one."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert (np.isnan(got) == np.isnan(ref)).all(), f"{what}: {int(np.isnan(got).sum())} NaN left"
    if not got.size:
        return
    tol = (k_c + 3) * DF.EPS * S
    err = np.abs(got - ref)
    ok = np.isnan(ref) | (err <= tol)
    ratio = np.nanmax(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)))
    print(f"  {family}, {what}: worst error / bound {ratio:.3f}")
    assert ok.all(), f"{what}: {int((~ok).sum())} elements over the bound, worst {ratio:.3f} x"


def check_silu(got, ref, cpu32, what, family):
    """rtol 1e-5, atol 1e-5 x max |ref| -- after CPU fp32 torch of the same pre-activation has passed it."""
    assert not np.isnan(got).any(), f"{what}: NaN left"
    if not got.size:
        return
    tol = 1e-5 * np.abs(ref).max() + 1e-5 * np.abs(ref)
    assert (np.abs(cpu32 - ref) <= tol).all(), f"{what}: CPU fp32 misses the criterion: the inputs are wrong"
    def worst(v):
        err = np.abs(v - ref)
        return float(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)).max())
    ratio = worst(got)
    print(f"  {family}, {what}: worst error / tolerance {ratio:.3f} (CPU fp32: {worst(cpu32):.3f})")
    assert ratio <= 1.0, f"{what}: worst {ratio:.3f} x the tolerance"


# ------------------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("case", DF.DENSE, ids=lambda c: c.id)
def test_dense_form_matches_fp64(case):
    c = case
    ops = DF.dense_operands(c)
    ref = DF.dense_reference(c, ops)
    a = c.n_act
    x_buf, x = guarded(ops["x"].shape[0], c.k, c.x_pad, c.x_off, ops["x"])
    assert DF.dense_form_of(c) == c.form
    assert hip.dense_form(c.n_rows, c.n_out, c.k, max(x.stride(0), c.k), x.data_ptr() % 16 == 0) == \
        (c.form[1], int(c.form[2] == "vec"))
    w = dev(ops["w"])
    packed = hip.dense_pack(w.t(), transpose=True) if c.tpack else hip.dense_pack(w)
    assert not c.tpack or w.t().stride(1) != 1 or c.k == 1
    bias = dev(ops["bias"]) if c.bias else None
    gather = dev(ops["gather"]) if ops["gather"] is not None else None
    fixed = [(x_buf, x)]
    kw = {}
    for name, pad in (("dpre", c.dpre), ("add", c.add)):
        if pad is not None:
            b, v = guarded(c.n_rows, a if name == "dpre" else c.n_out, pad, 0, ops[name])
            fixed.append((b, v))
            kw[name] = v
    pre_buf = pre = None
    if c.pre is not None:
        pre_buf, pre = guarded(c.n_rows, a, c.pre)
        kw["pre"] = pre
    if c.readout is not None:
        b_, n_, H_, C_ = c.readout
        assert c.n_rows == b_ * n_ and c.n_out == H_ * C_
        out_buf, flat = guarded(1, b_ * H_ * n_ * C_)
        out = flat.view(b_, H_, n_, C_)
        kw["out_map"] = DF.readout_map(*c.readout)
        offsets = torch.from_numpy(DF.scatter_map(c.n_rows, c.n_out, kw["out_map"])).cuda()
        assert offsets.unique().numel() == c.n_rows * c.n_out == flat.numel()      # a bijection: every element written once
        logical = lambda: flat[0][offsets]                                          # noqa: E731
        written = flat
    else:
        out_buf, out = guarded(c.n_rows, c.n_out, sum(c.out), c.out[0])
        logical = lambda: out                                                       # noqa: E731
        written = out
    before = {id(b): b.clone() for b in [out_buf, pre_buf] + [f[0] for f in fixed] if b is not None}
    launch(hip.dense, x, packed, c.n_out, c.k, n_rows=c.n_rows, bias=bias, gather=gather, row_mod=c.row_mod,
           activation=c.act, n_act=a, dropout_p=c.p, seed=c.seed, drop_width=DF.drop_width(c), out=out, **kw)
    assert torch.equal(outside(out_buf, out_buf, written), outside(before[id(out_buf)], out_buf, written)), "wrote outside out"
    if pre is not None:
        assert torch.equal(outside(pre_buf, pre_buf, pre), outside(before[id(pre_buf)], pre_buf, pre)), "wrote outside pre"
    for b, _ in fixed:
        assert torch.equal(b.view(torch.int32), before[id(b)].view(torch.int32)), "wrote an input"
    got = np64(logical())
    add = ops["add"].astype(np.float64) if c.add is not None else np.zeros((c.n_rows, c.n_out))
    if c.p > 0 and a:                                                                # the mask: exactly the Philox's
        if c.p < 1:
            assert c.positive and (ref["out"][:, :a] - add[:, :a])[ref["kf"] != 0].min() > 0.01     # no kept value is 0
        zeroed = got[:, :a] == add[:, :a]
        assert (zeroed == (ref["kf"] == 0)).all(), \
            f"dropout mask: {int((zeroed != (ref['kf'] == 0)).sum())} of {zeroed.size} positions differ from the Philox's"
    smooth = c.act == "silu" and a > 0
    if smooth:
        check_silu(got[:, :a], ref["out"][:, :a], ref["cpu32"], f"{c.id} silu columns", "dense silu")
    lin = slice(a if smooth else 0, None)
    check_bound(got[:, lin], ref["out"][:, lin], ref["S"][:, lin], c.k, f"{c.id} out", "dense")
    if pre is not None:
        check_bound(np64(pre), ref["pre"], ref["preS"], c.k, f"{c.id} pre", "dense")


# ------------------------------------------------------------------------------------------------------------ wgrad
@pytest.mark.parametrize("case", DF.WGRAD, ids=lambda c: c.id)
def test_dense_wgrad_form_matches_fp64(case):
    c = case
    ops = DF.wgrad_operands(c)
    ref = DF.wgrad_reference(c, ops)
    assert DF.wgrad_form_of(c) == c.form
    # (an empty tensor has no address: without rows the operands are one-row buffers and n_rows says 0)
    dz_buf, dz = guarded(max(c.n_rows, 1), c.n_out, c.dz_pad, 0)
    dz[:c.n_rows].copy_(torch.from_numpy(ops["dz"]))
    x_buf, x = guarded(max(ops["x"].shape[0], 1), c.k, 0, 0)
    x[:ops["x"].shape[0]].copy_(torch.from_numpy(ops["x"]))
    gather = dev(ops["gather"]) if ops["gather"] is not None else None
    dw_buf, dw = guarded(c.n_out, c.k, c.dw_pad)
    db_buf, db2 = guarded(1, c.n_out)
    db = db2[0] if c.bias else None
    before = [b.clone() for b in (dz_buf, x_buf, dw_buf, db_buf)]
    launch(hip.dense_wgrad, dz, x, c.n_out, c.k, n_rows=c.n_rows, gather=gather, row_mod=c.row_mod, bias=c.bias, dw=dw, db=db)
    assert torch.equal(outside(dw_buf, dw_buf, dw), outside(before[2], dw_buf, dw)), "wrote outside dw"
    if c.bias:
        assert torch.equal(outside(db_buf, db_buf, db2), outside(before[3], db_buf, db2)), "wrote outside db"
    else:
        assert torch.equal(db_buf.view(torch.int32), before[3].view(torch.int32)), "db written without a bias"
    assert torch.equal(dz_buf.view(torch.int32), before[0].view(torch.int32)) and \
        torch.equal(x_buf.view(torch.int32), before[1].view(torch.int32)), "wrote an input"
    rps, slices = DF.wgrad_rule(c.n_rows, c.n_out, c.k + int(c.bias))
    check_bound(np64(dw), ref["dw"], ref["dwS"], rps + slices, f"{c.id} dw", "wgrad")
    if c.bias:
        check_bound(np64(db), ref["db"], ref["dbS"], rps + slices, f"{c.id} db", "wgrad")
    first = (dw.clone(), db.clone() if c.bias else None)
    dw.fill_(float("nan"))
    launch(hip.dense_wgrad, dz, x, c.n_out, c.k, n_rows=c.n_rows, gather=gather, row_mod=c.row_mod, bias=c.bias, dw=dw, db=db)
    assert torch.equal(dw.view(torch.int32), first[0].view(torch.int32)), "two calls differ"
    assert not c.bias or torch.equal(db.view(torch.int32), first[1].view(torch.int32)), "two calls differ (db)"


# ------------------------------------------------------------------------------------------------------- row_segsum
@pytest.mark.parametrize("case", DF.SEGSUM, ids=lambda c: c.id)
def test_row_segsum_matches_fp64(case):
    c = case
    g_np = DF.rng_of(c.id).standard_normal((c.n_rows, c.width)).astype(np.float32)
    g_buf, g = guarded(c.n_rows, c.width, c.g_pad, 0, g_np)
    before = g_buf.clone()
    if c.mode == "strided":
        node = np.arange(c.n_rows) % c.n_seg
        out = launch(hip.row_segsum, g, c.n_seg)
    else:
        rng = DF.rng_of(c.id + "/nodes")
        node = np.full(c.n_rows, 2) if c.mode == "one" else 2 * rng.integers(0, c.n_seg // 2, c.n_rows)    # odd nodes: no rows
        keys, perm = torch.sort(torch.from_numpy(node), stable=True)
        out = launch(hip.row_segsum, g, c.n_seg, perm.to(torch.int32).cuda(), keys.to(torch.int32).cuda())
    assert torch.equal(g_buf.view(torch.int32), before.view(torch.int32)), "wrote its input"
    ref, S = np.zeros((c.n_seg, c.width)), np.zeros((c.n_seg, c.width))
    np.add.at(ref, node, g_np.astype(np.float64))
    np.add.at(S, node, np.abs(g_np).astype(np.float64))
    longest = int(np.bincount(node, minlength=1).max()) if c.n_rows else 0
    check_bound(np64(out), ref, S, longest, c.id, "row_segsum")
    if c.mode != "strided":
        empty = np.setdiff1d(np.arange(c.n_seg), node)
        assert empty.size and not np64(out)[empty].any()                  # nodes without rows: zero


# ------------------------------------------------------------------------------------------------------- masked_mae
@pytest.mark.parametrize("case", DF.MAE, ids=lambda c: c.id)
def test_masked_mae_matches_fp64(case):
    c = case
    rng = DF.rng_of(c.id)
    yh, y = rng.standard_normal(c.n).astype(np.float32), rng.standard_normal(c.n).astype(np.float32)
    y[::5] = yh[::5]                                                     # y_hat == y: gradient 0
    if c.nans:
        y[2::11] = np.nan
    mask = (rng.random(c.n) < 0.7) if c.mask else None
    d32 = yh - y                                                          # (the sign of the fp32 difference is the fp64 one's)
    counts = np.ones(c.n, bool) if mask is None else mask.copy()
    if c.mask_nans:
        counts &= ~np.isnan(d32)
    total = np.abs(yh.astype(np.float64) - y.astype(np.float64))[counts].sum()
    n_counted = int(counts.sum())
    want = total / n_counted if n_counted else 0.0
    m = dev(mask.astype(np.uint8)) if mask is not None else None
    flat = lambda t: None if t is None else t.view(1, 1, c.n)             # noqa: E731  ([B, H, row]: one flat row)
    loss, count = launch(hip.masked_loss, flat(dev(yh)), flat(dev(y)), flat(m), "mae", None, c.mask_nans)
    assert float(count.item()) == n_counted
    got = float(loss.item())
    if np.isnan(want):
        assert np.isnan(got)
    else:
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    grad = launch(hip.masked_loss_bwd, flat(dev(yh)), flat(dev(y)), flat(m), "mae", None, c.mask_nans,
                  torch.tensor([c.grad_out], device="cuda"), count).view(-1)
    scale = np.float32(c.grad_out) / np.float32(max(n_counted, 1))
    sign = np.where(np.isnan(d32), np.nan, np.sign(d32)).astype(np.float64)
    ref = np.where(counts, sign * float(scale), 0.0)
    check_bound(np64(grad), ref, np.abs(np.nan_to_num(ref)), 0, f"{c.id} grad", "masked_mae_bwd")
    if c.n:
        assert (np64(grad)[(d32 == 0)] == 0).all()


# ---------------------------------------------------------------------------------------------------- grouped layer
def grouped_rows(c, ops):
    """(buffer, x2, source) on the device with the case's strides."""
    D = c.groups * c.ic
    if c.src is None:
        buf, x2 = guarded(max(c.n_rows, 1), D, c.x_pad, c.x_off)
        x2[:c.n_rows].copy_(torch.from_numpy(ops["x"]))
        return buf, x2[:c.n_rows] if c.n_rows else x2[:0], None
    T, N, bpad = c.src
    rs = D + c.x_pad
    size = T * (N * rs + bpad)
    buf = torch.full((GUARD + size + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    src = torch.as_strided(buf, (T, N, D), (N * rs + bpad, rs, 1), GUARD)
    src.copy_(torch.from_numpy(ops["x"]))
    return buf, None, src


@pytest.mark.parametrize("case", DF.GROUPED, ids=lambda c: c.id)
def test_grouped_layer_form_matches_fp64(case):
    c = case
    ops = DF.grouped_operands(c)
    ref = DF.grouped_reference(c, ops)
    assert DF.grouped_form_of(c) == set(c.forms)
    width, seed = c.groups * c.oc, DF.grouped_seed(c)
    buf, x2, src = grouped_rows(c, ops)
    before = buf.clone()
    w = dev(ops["w"])
    packed = hip.grouped_linear_pack(w, c.groups)
    step, node = (dev(ops["step"]), dev(ops["node"])) if src is not None else (None, None)
    if c.n_rows == 0:                                                    # no rows: a zero gradient (the binding's own answer)
        empty = torch.empty(0, dtype=torch.int32, device="cuda")
        dw = launch(hip.grouped_linear_wgrad, None, torch.empty(0, width, device="cuda"), c.groups, c.ic, c.oc,
                    step_index=empty, node_index=empty, source=src)
        assert tuple(dw.shape) == (width, c.ic) and not bool(dw.any())
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "wrote its input"
        return
    out, pre = launch(hip.grouped_linear, x2, packed, dev(ops["bias"]), c.groups, c.ic, c.oc, c.act, step_index=step,
                      node_index=node, source=src, want_pre=True, dropout_p=c.p, seed=seed)
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "wrote its input"
    got = np64(out)
    if c.p:                                                              # index row * groups * oc + g * oc + j
        assert np.abs(ref["out"])[ref["kf"] != 0].min() > 0.1             # positive operands: no kept value is 0
        assert ((got == 0) == (ref["kf"] == 0)).all(), "dropout mask differs from the Philox's"
    check_bound(np64(pre), ref["pre"], ref["S"], c.ic, f"{c.id} pre", "grouped")
    if c.act == "silu":
        check_silu(got, ref["out"], ref["cpu32"], f"{c.id} out", "grouped silu")
    else:
        check_bound(got, ref["out"], ref["S"] * ref["kf"], c.ic, f"{c.id} out", "grouped")
    # dact: a strided dy, act' at the pre the forward stored, the same mask
    dy_buf, dy = guarded(c.n_rows, width, 3, 0, ops["dy"])
    dz = launch(hip.grouped_linear_dact, dy, pre, c.act, dropout_p=c.p, seed=seed)
    assert dz.is_contiguous() and tuple(dz.shape) == (c.n_rows, width)
    pre_got = pre.cpu().numpy()
    dy64 = ops["dy"].astype(np.float64)
    dz_ref = dy64 * DF.dact64(pre_got.astype(np.float64), c.act) * ref["kf"]
    if c.p:
        assert np.abs(dz_ref)[ref["kf"] != 0].min() > 0.1                 # |dy| >= 1/2 and act'(pre > 0) >= 1/2
        assert ((np64(dz) == 0) == (ref["kf"] == 0)).all(), "dact: dropout mask differs from the Philox's"
    if c.act == "silu":
        check_silu(np64(dz), dz_ref, (ops["dy"] * DF.dact32(pre_got, c.act) * ref["kf"]).astype(np.float64),
                   f"{c.id} dact", "grouped silu")
    else:
        check_bound(np64(dz), dz_ref, np.abs(dz_ref), 0, f"{c.id} dact", "grouped")
    # transpose: per group, torch.transpose
    wt = launch(hip.grouped_linear_transpose, w, c.groups)
    assert torch.equal(wt, w.reshape(c.groups, c.oc, c.ic).transpose(1, 2).reshape(c.groups * c.ic, c.oc))
    # wgrad of the dz just computed
    dw = launch(hip.grouped_linear_wgrad, x2, dz, c.groups, c.ic, c.oc, step_index=step, node_index=node, source=src)
    dw_ref, dwS = DF.grouped_wgrad_reference(c, ref["rows"], dz.cpu().numpy())
    rps, slices = hip.grouped_linear_wgrad_form(c.n_rows, c.groups, c.ic, c.oc)
    check_bound(np64(dw), dw_ref, dwS, rps + slices, f"{c.id} dw", "grouped wgrad")
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "wrote its input"


# ---------------------------------------------------------------------------------------------------- the bindings
class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: the binding has to refuse before any launch")


def test_bindings_refuse_overlapping_rows_and_strided_operands(monkeypatch):
    """``_rows2``: an expanded view (rows 0 floats apart) is refused, not read as rows ``width`` apart;
    ``grouped_linear_wgrad``: dz has to be the contiguous [K, groups * oc] tensor the kernel indexes;
    ``grouped_linear_dact``: pre has to be contiguous (dz and pre are indexed flat).  All before a launch."""
    assert not _device_error
    w = torch.randn(8, 8, device="cuda")
    packed = hip.dense_pack(w)
    one = torch.randn(1, 8, device="cuda")
    real = torch.randn(4, 8, device="cuda")
    x2 = torch.randn(4, 6, device="cuda")
    wide = torch.randn(4, 12, device="cuda")
    monkeypatch.setattr(hip, "require_gpu", lambda: _NoLaunch())
    with pytest.raises(ValueError, match="overlap"):
        hip.dense(one.expand(4, 8), packed, 8, 8)
    with pytest.raises(ValueError, match="overlap"):
        hip.dense(real, packed, 8, 8, add=one.expand(4, 8))
    with pytest.raises(ValueError, match="overlap"):
        hip.dense_wgrad(one.expand(4, 8), real, 8, 8)
    with pytest.raises(ValueError, match="overlap"):
        hip.row_segsum(one.expand(4, 8), 2)
    with pytest.raises(ValueError, match="dz"):
        hip.grouped_linear_wgrad(x2, wide[:, :10], 2, 3, 5)                # [4, 10] but rows 12 floats apart
    with pytest.raises(ValueError, match="dz"):
        hip.grouped_linear_wgrad(x2, torch.randn(4, 12, device="cuda"), 2, 3, 5)     # wrong width
    with pytest.raises(ValueError, match="dz"):
        hip.grouped_linear_wgrad(x2, torch.randn(4, 10, device="cuda").double(), 2, 3, 5)
    with pytest.raises(ValueError, match="pre"):
        hip.grouped_linear_dact(real, wide[:, :8], "relu")
    monkeypatch.undo()
    # one row may have any stride, and an expanded gradient goes through the layers' own copy (nn/dense.rows2d)
    from sgp_amd.nn import dense
    y = hip.dense(one.expand(1, 8), packed, 8, 8)
    torch.cuda.synchronize()
    assert torch.allclose(y, one @ w.T, rtol=1e-5, atol=1e-5)
    e = dense.rows2d(one.expand(4, 8))
    assert e.stride(0) == 8 and torch.equal(e, one.expand(4, 8)) and dense.rows2d(real) is real
