"""sgp_amd.connectivity on the host: argument errors come before any GPU need, there is no CPU fallback, and the numpy
restatement the GPU tests compare against gives the hand-worked answers on 4-node cases."""
import numpy as np
import pytest
import torch

import connectivity_ref as ref
import sgp_amd
from sgp_amd import connectivity, hip


LATLON = torch.tensor([[40.0, -100.0], [40.5, -100.0], [41.0, -99.0], [39.0, -101.0]], dtype=torch.float64)


def test_exports():
    for name in ("geographic_connectivity", "correntropy_similarity", "dense_connectivity", "correntropy_connectivity"):
        assert getattr(sgp_amd, name) is getattr(connectivity, name)


def test_knn_limit_matches_the_library():
    if not hip.os.path.exists(hip.LIB_PATH):
        hip.build()
    assert connectivity.MAX_KNN == hip.conn_max_knn() >= 512


@pytest.mark.parametrize("call", [
    lambda: sgp_amd.geographic_connectivity(torch.zeros(4, 3), 50.0, knn=2),
    lambda: sgp_amd.geographic_connectivity(torch.zeros(4), 50.0, knn=2),
    lambda: sgp_amd.geographic_connectivity(torch.zeros(0, 2), 50.0),
    lambda: sgp_amd.geographic_connectivity(LATLON, 0.0, knn=2),
    lambda: sgp_amd.geographic_connectivity(LATLON, 50.0, knn=5),                       # knn > N
    lambda: sgp_amd.geographic_connectivity(LATLON, 50.0, knn=0),
    lambda: sgp_amd.geographic_connectivity(LATLON, 50.0, knn=2, layout="dense"),
    lambda: sgp_amd.geographic_connectivity(LATLON, 50.0, knn=2, layout="coo"),
    lambda: sgp_amd.geographic_connectivity(LATLON, 50.0, knn=2, normalize_axis=2),
    lambda: sgp_amd.dense_connectivity(torch.zeros(4, 5), knn=2),
    lambda: sgp_amd.dense_connectivity(torch.zeros(4, 4, dtype=torch.int64), knn=2),
    lambda: sgp_amd.dense_connectivity(torch.zeros(4, 4), knn=5),
    lambda: sgp_amd.correntropy_similarity(torch.zeros(7, 3), 7, 0.05),                 # T <= period: no chunk
    lambda: sgp_amd.correntropy_similarity(torch.zeros(5, 3), 7, 0.05),
    lambda: sgp_amd.correntropy_similarity(torch.zeros(20), 7, 0.05),
    lambda: sgp_amd.correntropy_connectivity(torch.zeros(7, 3), 7, 0.05, knn=2),
    lambda: sgp_amd.correntropy_connectivity(torch.zeros(20, 3), 7, 0.05, knn=4),
])
def test_argument_errors_come_first(call):
    with pytest.raises(ValueError):
        call()


def test_knn_over_the_limit_names_it():
    n = connectivity.MAX_KNN + 10
    with pytest.raises(NotImplementedError, match=str(connectivity.MAX_KNN)):
        sgp_amd.geographic_connectivity(torch.zeros(n, 2), 50.0, knn=connectivity.MAX_KNN + 1)
    with pytest.raises(NotImplementedError, match=str(connectivity.MAX_KNN)):
        sgp_amd.dense_connectivity(torch.zeros(n, n), knn=connectivity.MAX_KNN + 1)


def test_library_rejects_bad_arguments_without_a_device():
    if not hip.os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.load()
    inf = float("-inf")
    assert lib.sgp_conn_geo_knn_f64(None, 4, 2, 0, 0, inf, 1.0, 1.0, None, None, None) == hip.SGP_EINVAL
    assert b"null pointer" in lib.sgp_last_error()
    buf = torch.zeros(64, dtype=torch.float64)
    p = buf.data_ptr()
    assert lib.sgp_conn_geo_knn_f64(p, 4, 5, 0, 0, inf, 1.0, 1.0, p, p, None) == hip.SGP_EINVAL
    assert lib.sgp_conn_dense_knn(p, 1, 1000, 1, 1000, 513, 0, 0, inf, p, p, None) == hip.SGP_EUNSUP
    assert b"512" in lib.sgp_last_error()
    assert lib.sgp_conn_geo_rows_f64(p, 4, 0, 0, inf, 2.0, 1.0, 1.0, p, None, None, None, None) == hip.SGP_EINVAL
    assert lib.sgp_correntropy_f32(p, 2, 4, 7, 1, 0.05, p, p, 4, None) == hip.SGP_EINVAL      # row stride < n


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sgp_amd.geographic_connectivity(LATLON, 50.0, knn=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sgp_amd.dense_connectivity(torch.eye(4), knn=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sgp_amd.correntropy_similarity(torch.randn(20, 3), 7, 0.05)


# ---- the restatement on hand-worked 4-node cases
SIM = np.array([[1.0, 0.5, 0.2, 0.0],
                [0.5, 1.0, 0.5, 0.1],
                [0.2, 0.7, 1.0, 0.7],
                [0.0, 0.1, 0.3, 1.0]])


def test_ref_knn_edge_order_and_ties():
    # row 1 ties 0.5 between columns 0 and 2 -> column 0; row 2 ties 0.7 between columns 1 and 3 -> column 1
    (ei, ew), _ = ref.connectivity(SIM, knn=1, include_self=False)
    # entries A[0,1], A[1,0], A[2,1], A[3,2]; as (source j, target i) ordered by (j, i)
    assert ei.tolist() == [[0, 1, 1, 2], [1, 0, 2, 3]]
    assert ew.tolist() == [np.float32(0.5), np.float32(0.5), np.float32(0.7), np.float32(0.3)]
    assert ei.dtype == np.int64 and ew.dtype == np.float32


def test_ref_include_self_keeps_the_loop():
    (ei, ew), _ = ref.connectivity(SIM, knn=1, include_self=True)
    assert ei.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]] and ew.tolist() == [1.0] * 4
    (rowptr, col, val), _ = ref.connectivity(SIM, knn=2, include_self=True, layout="csr")
    assert rowptr.tolist() == [0, 2, 4, 6, 8]
    assert col.tolist() == [0, 1, 0, 1, 1, 2, 2, 3]                    # rows 1 and 2: the tie goes to the lower column
    assert val.tolist() == [1.0, 0.5, 0.5, 1.0, np.float32(0.7), 1.0, np.float32(0.3), 1.0]


def test_ref_threshold_binary_symmetric_normalize():
    (rowptr, col, val), _ = ref.connectivity(SIM, threshold=0.25, include_self=False, layout="csr")
    assert rowptr.tolist() == [0, 1, 3, 5, 6] and col.tolist() == [1, 0, 2, 1, 3, 2]
    # binary with knn: exactly k ones per row, whatever the value (row 0 keeps the 0.2; its 0.0 is never reached)
    dense, _ = ref.connectivity(SIM, knn=2, binary_weights=True, include_self=False, layout="dense")
    assert dense.tolist() == [[0, 1, 1, 0], [1, 0, 1, 0], [0, 1, 0, 1], [0, 1, 1, 0]]
    # binary without knn: sim > 0
    dense, _ = ref.connectivity(SIM, binary_weights=True, include_self=False, layout="dense")
    assert dense.tolist() == [[0, 1, 1, 0], [1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 0]]
    # union of both directions, the larger weight
    dense, _ = ref.connectivity(SIM, knn=1, include_self=False, force_symmetric=True, layout="dense")
    want = np.zeros((4, 4), dtype=np.float32)
    want[0, 1] = want[1, 0] = 0.5
    want[1, 2] = want[2, 1] = 0.7
    want[2, 3] = want[3, 2] = 0.3
    assert np.array_equal(dense, want)
    # rows sum to 1 (up to epsilon); axis 0 is the reference's no-op
    dense, _ = ref.connectivity(SIM, knn=2, include_self=False, normalize_axis=1, layout="dense")
    assert np.allclose(dense.sum(1), 1.0, atol=1e-6)
    a0, _ = ref.connectivity(SIM, knn=2, include_self=False, normalize_axis=0, layout="dense")
    a, _ = ref.connectivity(SIM, knn=2, include_self=False, layout="dense")
    assert np.array_equal(a0, a)
    # knn = N without the diagonal keeps the N - 1 others
    dense, _ = ref.connectivity(SIM + 1.0, knn=4, include_self=False, layout="dense")
    assert (dense != 0).sum(1).tolist() == [3, 3, 3, 3]


def test_ref_geographic_and_correntropy():
    sim = ref.geographic_similarity(LATLON.numpy(), 50.0)
    assert np.array_equal(np.diag(sim), np.ones(4)) and np.allclose(sim, sim.T)
    # one degree of latitude is 111.195 km on this sphere: nodes 0 and 1 are half a degree apart
    d01 = np.sqrt(-np.log(sim[0, 1])) * 50.0
    assert abs(d01 - np.pi * ref.EARTH_RADIUS_KM / 360.0) < 1e-9
    rng = np.random.default_rng(0)
    x = rng.standard_normal((21, 3))
    s = ref.correntropy_similarity(x, 7, 0.05)              # chunks end at 7 and 14; the one ending at T = 21 is dropped
    z = (x - x.mean()) / x.std()
    want = np.mean([np.exp(-0.05 * ((z[lo:lo + 7, 0] - z[lo:lo + 7, 1]) ** 2).sum()) for lo in (0, 7)])
    assert abs(s[0, 1] - want) < 1e-12 and np.array_equal(np.diag(s), np.ones(3))
    with pytest.raises(ValueError):
        ref.correntropy_similarity(x[:7], 7, 0.05)
