"""Engine.top_k on the GPU (docs/TOPK.md): one engine each of six of tests/test_gpu_predict.py's families after three iterations -- the result against
get_factors' W and H through the tolerant check of tests/topk_reference.py on both axes, host arrays against device tensors bit for bit, exclusion of the
training entries, the side effects against get_factors' (the trajectory and the error of the last error iteration), and the refusals.

The bound of check_top_k is the standard one of an r-term dot product in any order, gamma_r(u) sum_k |w_k h_k| with u = 2^-24 or 2^-53; nothing is measured."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import topk_reference as tref
from tests.test_gpu_predict import FAMILIES, U, bits, engine, errors_of, on_device, problem, torch_

pytestmark = pytest.mark.gpu

NAMES = ["mu_r7_pending_scale", "mu_r70", "mu_r200", "mu_f64_r70", "nsnmf", "masked_frobenius"]
NQ, K = 45, 10


def query_list(count, seed):
    """NQ indices below count: unsorted, a duplicate, both ends."""
    q = np.random.default_rng(seed).integers(0, count, NQ).astype(np.int32)
    q[0], q[-1], q[3] = 0, count - 1, q[2]
    return q


@pytest.mark.parametrize("name", NAMES)
def test_top_k_of_a_family(name):
    (m, n), r, dtype, _, _, _ = FAMILIES[name]
    p = problem(name)
    u = U[dtype]
    eng, twin = engine(name), engine(name)
    before = errors_of(eng, name)
    qr, qc = query_list(m, 1), query_list(n, 2)
    idx, sc = eng.top_k(qr, K)
    assert idx.dtype == np.int32 and sc.dtype == dtype and idx.shape == sc.shape == (NQ, K)
    assert errors_of(eng, name) == before, "the error of the last error iteration moved"
    # against the factors of get_factors -- the twin's, which ran the same three iterations: this engine goes on with nothing but top_k behind it
    W, H = twin.get_factors()
    W64, Ht64 = W.astype(np.float64), np.ascontiguousarray(H.T.astype(np.float64))
    tref.check_top_k(idx, sc, W64, Ht64, qr, K, None, 0, u)
    # the effects are get_factors': the twin took get_factors where this engine took top_k, and both go on
    eng.iterate(2, first_iteration=4, error_every=1)
    twin.iterate(2, first_iteration=4, error_every=1)
    (W2, H2), (Wt2, Ht2) = eng.get_factors(), twin.get_factors()
    assert bits(W2) == bits(Wt2) and bits(H2) == bits(Ht2), "top_k disturbed the trajectory where get_factors does not"
    assert errors_of(eng, name) == errors_of(twin, name)
    W64, Ht64 = W2.astype(np.float64), np.ascontiguousarray(H2.T.astype(np.float64))
    torch = torch_()
    rows, cols = (a.astype(np.int32) for a in np.nonzero(p["mask"]))      # the training entries (of the masked family; the same pattern elsewhere)
    for axis, q, count, Aq, Bc in ((0, qr, n, W64, Ht64), (1, qc, m, Ht64, W64)):
        idx, sc = eng.top_k(q, K, axis=axis)
        tref.check_top_k(idx, sc, Aq, Bc, q, K, None, 0, u)
        # a repeated call, index base 1 and the device form: the same bits
        again = eng.top_k(q, K, axis=axis)
        assert bits(again[0]) == bits(idx) and bits(again[1]) == bits(sc)
        one = eng.top_k(q + 1, K, axis=axis, base=1)
        assert bits(one[0]) == bits(idx + 1) and bits(one[1]) == bits(sc)
        d_idx, d_sc = eng.top_k(on_device(q), K, axis=axis)
        assert isinstance(d_idx, torch.Tensor) and d_idx.is_cuda and d_sc.is_cuda and tuple(d_idx.shape) == (NQ, K)
        assert bits(d_idx.cpu().numpy()) == bits(idx) and bits(d_sc.cpu().numpy()) == bits(sc)
        # the training entries excluded: none comes back, and what comes back is the top of the rest
        excl = na.exclusion_lists(q, rows, cols, axis=axis)
        e_idx, e_sc = eng.top_k(q, K, axis=axis, exclude=excl)
        tref.check_top_k(e_idx, e_sc, Aq, Bc, q, K, excl, 0, u)
        pairs = p["mask"][q[:, None], e_idx] if axis == 0 else p["mask"][e_idx, q[:, None]]
        assert np.all(e_idx >= 0) and not pairs.any(), "a training entry came back"
        assert not np.array_equal(e_idx, idx), "the exclusion changed nothing"
        d_idx, d_sc = eng.top_k(on_device(q), K, axis=axis, exclude=(on_device(excl[0]), on_device(excl[1])))
        assert bits(d_idx.cpu().numpy()) == bits(e_idx) and bits(d_sc.cpu().numpy()) == bits(e_sc)
    # k = 64 and a query whose list leaves fewer than k
    q1 = qr[:3]
    ptr = np.array([0, 0, n - 5, n - 5], np.int64)
    lst = np.random.default_rng(3).permutation(n)[:n - 5].astype(np.int32)
    idx, sc = eng.top_k(q1, 64, exclude=(ptr, lst))
    tref.check_top_k(idx, sc, W64, Ht64, q1, 64, (ptr, lst), 0, u)
    assert np.sum(idx[1] >= 0) == 5 and np.all(idx[1, 5:] == -1) and np.all(np.isneginf(sc[1, 5:]))
    eng.close(); twin.close()


def test_refusals():
    name = "mu_r70"
    (m, n), r, dtype, _, _, _ = FAMILIES[name]
    eng = engine(name)
    torch = torch_()
    q = query_list(m, 1)
    ptr = np.arange(NQ + 1, dtype=np.int64); lst = np.arange(NQ, dtype=np.int32)

    def refused(call, *words):
        with pytest.raises(na.EngineError) as err:
            call()
        assert err.value.status == 1
        for w in words:
            assert w in str(err.value), (w, str(err.value))

    # a query outside its range: the first bad one is named; on the device path the validation launch stops the product
    bad = q.copy(); bad[[7, 30]] = m
    refused(lambda: eng.top_k(bad, K), "query 7 ", "outside", "on the host")
    refused(lambda: eng.top_k(q, K, base=1), "query 0 ", "outside")      # (q[0] = 0 lies below base 1)
    far = query_list(n, 2); far[-1] = n      # inside the rows, outside the columns
    assert n < m and eng.top_k(far, K)[0].shape == (NQ, K)
    refused(lambda: eng.top_k(far, K, axis=1), f"query {NQ - 1} ", "outside")
    s_idx = torch.full((NQ * K,), -7, dtype=torch.int32, device="cuda")
    s_sc = torch.full((NQ * K,), float("nan"), dtype=torch.float32, device="cuda")
    d_bad = on_device(bad)
    st = eng._lib.nmfamd_engine_top_k_device(eng._h, C.c_void_p(d_bad.data_ptr()), C.c_long(NQ), K, 0, 0, None, None, C.c_long(0), C.c_void_p(s_idx.data_ptr()),
                                             C.c_void_p(s_sc.data_ptr()))
    text = eng._lib.nmfamd_engine_last_error(eng._h).decode()
    assert st == 1 and "query 7 " in text and "outside" in text and "the product was not launched" in text
    torch.cuda.synchronize()
    assert bool((s_idx == -7).all()) and bool(torch.isnan(s_sc).all()), "a product wrote results behind a failed validation"
    refused(lambda: eng.top_k(on_device(bad), K), "query 7 ", "not launched")
    # an excluded index outside the candidates; a malformed excl_ptr
    refused(lambda: eng.top_k(q, K, exclude=(ptr, lst + (n - 10))), f"excluded index 10 ", "outside", "on the host")
    refused(lambda: eng.top_k(q, K, exclude=(ptr, lst - 1)), "excluded index 0 ")
    refused(lambda: eng.top_k(q, K, exclude=(ptr + 1, np.arange(NQ + 1, dtype=np.int32))), "excl_ptr", "at 0 ")
    down = ptr.copy(); down[20] = 5
    refused(lambda: eng.top_k(q, K, exclude=(down, lst)), "excl_ptr", "at 20 ")
    d_q = on_device(q)
    refused(lambda: eng.top_k(d_q, K, exclude=(on_device(ptr), on_device(lst + (n - 10)))), "excluded index 10 ", "not launched")
    refused(lambda: eng.top_k(d_q, K, exclude=(on_device(down), on_device(lst))), "excl_ptr", "at 20 ", "not launched")
    refused(lambda: eng.top_k(d_q, K, exclude=(on_device(ptr), on_device(np.arange(NQ + 3, dtype=np.int32)))), "excl_ptr", f"at {NQ} ", "excl_nnz")
    # the numbers
    refused(lambda: eng.top_k(q[:0], K), "nq")
    refused(lambda: eng.top_k(q, 0), "k has to be")
    refused(lambda: eng.top_k(q, na.TOPK_MAX_K + 1), "k has to be")
    refused(lambda: eng.top_k(q, K, base=2), "base")
    refused(lambda: eng.top_k(q, K, axis=2), "axis")
    # host memory handed to the device entry
    out_i, out_s = np.zeros(NQ * K, np.int32), np.zeros(NQ * K, dtype)
    st = eng._lib.nmfamd_engine_top_k_device(eng._h, C.c_void_p(q.ctypes.data), C.c_long(NQ), K, 0, 0, None, None, C.c_long(0), C.c_void_p(out_i.ctypes.data),
                                             C.c_void_p(out_s.ctypes.data))
    assert st == 1 and "queries: not device memory" in eng._lib.nmfamd_engine_last_error(eng._h).decode()
    # after all that the engine still answers
    assert np.all(eng.top_k(q, K)[0] >= 0)
    eng.close()
    # an engine with row blocks holds a column shard; an engine without factors has nothing to rank
    blocks = na.Engine(300, 257, 7, "mu", row_blocks=2)
    blocks.randomize(3)
    refused(lambda: blocks.top_k(q, K), "row blocks")
    blocks.close()
    empty = na.Engine(300, 257, 7, "mu")
    refused(lambda: empty.top_k(q, K), "no factors")
    empty.randomize(3)
    assert np.all(empty.top_k(q, K)[0] >= 0)      # (no upload of V is needed)
    empty.close()
