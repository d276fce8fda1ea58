"""Every packing entry that writes the fragment order of csrc/frag.h, through its binding, against the layout written
by hand (tests/frag_layout.py): bit for bit, at the smallest shapes with one tile, a ragged tile and more than one
k-block.  (``hip.grin_pack`` has the same comparison in tests/test_gpu_grin_forms.py.)"""
import numpy as np
import pytest
import torch

from frag_layout import pack_one, unpack_one
from sgp_amd import hip

pytestmark = pytest.mark.gpu


def draw(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return torch.equal(got, want)


@pytest.mark.parametrize("n_out,k", [(17, 18), (16, 16)])
def test_dense_pack_plain_and_transposed_view(n_out, k):
    w = draw(n_out, k, seed=n_out)
    assert same(hip.dense_pack(w.cuda()), pack_one(w.numpy(), 0))
    # M^T given as a [k, n_out] view whose rows lie n_out + 3 floats apart
    wide = draw(k, n_out + 3, seed=k + 1).cuda()
    view = wide[:, :n_out]
    assert not view.is_contiguous() and view.stride() == (n_out + 3, 1)
    got = hip.dense_pack(view, transpose=True)
    assert got.numel() == hip.load().sgp_dense_packed_floats(n_out, k)
    assert same(got, pack_one(view.cpu().numpy(), 1))


@pytest.mark.parametrize("H", [16, 48])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_rnn_window_pack_both_halves(cell, H):
    G = hip.RNN_GATES[cell]
    w = draw(G * H, H, seed=G + H)
    got = hip.rnn_window_pack(w.cuda(), cell)
    assert got.numel() == 2 * G * H * H
    assert same(got[:G * H * H], pack_one(w.numpy(), 0))               # forward: [G JT][JT]
    assert same(got[G * H * H:], pack_one(w.numpy(), 1))               # backward: [JT][G JT], transposed


@pytest.mark.parametrize("H,D", [(16, 1), (32, 17), (48, 16)])
def test_rnn_impute_pack_six_parts_and_zero_padding(H, D):
    DP = 16 * (-(-D // 16))
    w_ih = draw(3 * H, D + 3, seed=H + D)                              # W_x = the first D columns; the others must not leak
    w_hh, w_r = draw(3 * H, H, seed=H), draw(D, H, seed=D)
    got = hip.rnn_impute_pack(w_ih.cuda(), w_hh.cuda(), w_r.cuda(), D).cpu()
    srcs = [w_hh.numpy(), w_ih[:, :D].numpy(), w_r.numpy()]
    want = [pack_one(s, trans) for trans in (0, 1) for s in srcs]      # W_hh, W_x, W_r, then their transposes
    sizes = [3 * H * H, 3 * H * DP, DP * H] * 2
    assert [len(w) for w in want] == sizes and got.numel() == sum(sizes)
    at = 0
    for i, (w, n) in enumerate(zip(want, sizes)):
        assert same(got[at:at + n], w), f"part {i}"
        at += n
    # the D tiles are padded with zeros, not with what lies beside the matrix: rows / columns D .. DP - 1 of every part
    parts = torch.split(got, sizes)
    wx, wr = unpack_one(parts[1].numpy(), 3 * H, D), unpack_one(parts[2].numpy(), D, H)
    wxt, wrt = unpack_one(parts[4].numpy(), D, 3 * H), unpack_one(parts[5].numpy(), H, D)
    assert wx.shape == (3 * H, DP) and wr.shape == (DP, H) and wxt.shape == (DP, 3 * H) and wrt.shape == (H, DP)
    for pad, other in ((wx[:, D:], 3 * H), (wr[D:], H), (wxt[D:], 3 * H), (wrt[:, D:], H)):
        assert pad.size == (DP - D) * other and not pad.any()
    assert np.array_equal(wx[:, :D], srcs[1]) and np.array_equal(wrt[:, :D], srcs[2].T)
