"""What the C ABI's host-side input checks refuse, with which words, and what a refusal leaves behind.

The scorers and trainers that take node ids copy them to the host and compare every one against [0, N) before any
kernel reads them; the three entries that take a caller's CSR check it on the host once.  Every case here is one tiny
call on the 4-node path graph 0 - 1 - 2 - 3 with L = 3 links: a bad id at each place of the list, or a CSR broken in
one way.  A refusal is S3GRL_ERR_INVALID_ARGUMENT (ValueError) with the entry's own text, its outputs still hold the
sentinel they were filled with, and the same entry with valid input, called right afterwards, succeeds: the handle
and the context stay usable."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_NODES = 4
INDPTR = (0, 1, 3, 5, 6)
INDICES = (1, 0, 2, 1, 3, 2)
LINKS = ((0, 1, 0), (2, 3, 1))          # int32 [2, L]; read as [L, 2] pairs by the mf and linkclf entries
SOURCES = (0, 1)                        # Katz: the distinct sources of LINKS
CN_PTR, CN_TOTAL = (0, 1, 2, 2), 2      # the common-neighbour lists of LINKS: {1}, {2}, {}
PLACES = {"first row": 1, "second row": 3, "last element": 5}   # flat positions in the six ids
P, HLL_P, HOPS = 64, 7, 1               # the smallest sketch tables
DIM = 4


def _engine():
    from s3grl_amd.engine import default_engine

    return default_engine()


def _dev(values, dtype):
    return torch.as_tensor(np.asarray(values), dtype=dtype).to(_engine().device).contiguous()


def _sentinel(shape, dtype):
    fill = float("nan") if dtype.is_floating_point else (0xFF if dtype == torch.uint8 else -1)
    return torch.full(shape, fill, dtype=dtype, device=_engine().device)


def _untouched(t):
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t == (0xFF if t.dtype == torch.uint8 else -1)).all())


def _refused(status, what, text):
    from s3grl_amd import _native as N

    with pytest.raises(ValueError) as info:
        N.check(status, what)
    assert text in str(info.value), (what, str(info.value))


def _graph():
    return _dev(INDPTR, torch.int64), _dev(INDICES, torch.int32)


# ---- id checks ------------------------------------------------------------------------------------------------------

@contextmanager
def _heuristics():
    from s3grl_amd import _native as N

    ip, ix = _graph()
    h = C.c_void_p()
    N.check(N.lib().s3grl_heuristics_create(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), None, len(INDICES),
                                            C.byref(h)), "s3grl_heuristics_create")
    try:
        yield h
    finally:
        N.lib().s3grl_heuristics_destroy(h)


@contextmanager
def _pairs_entry(kind):
    from s3grl_amd import _native as N

    with _heuristics() as h:
        def call(links):
            out = _sentinel((3,), torch.float32)
            return N.lib().s3grl_heuristics_pairs(h, kind, N.ptr(links), 3, N.ptr(out)), [out]

        yield call, "s3grl_heuristics_pairs", "heuristics: a link endpoint outside [0, N)"


@contextmanager
def _katz_entry():
    from s3grl_amd import _native as N

    with _heuristics() as h:
        src = _dev(SOURCES, torch.int32)

        def call(links):
            out = _sentinel((3,), torch.float32)
            return N.lib().s3grl_heuristics_katz(h, N.ptr(src), len(SOURCES), N.ptr(links), 3, 0.05, 3, 0,
                                                 N.ptr(out)), [out]

        yield call, "s3grl_heuristics_katz", "heuristics: a link endpoint outside [0, N)"


@contextmanager
def _cn_count_entry():
    from s3grl_amd import _native as N

    ip, ix = _graph()

    def call(links):
        out = _sentinel((3,), torch.int64)
        return N.lib().s3grl_cn_count(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), len(INDICES), N.ptr(links), 3, 1,
                                      N.ptr(out)), [out]

    yield call, "s3grl_cn_count", "ncn: a link endpoint outside [0, N)"


@contextmanager
def _cn_fill_entry():
    from s3grl_amd import _native as N

    ip, ix = _graph()
    cn_ptr = _dev(CN_PTR, torch.int64)

    def call(links):
        out = _sentinel((CN_TOTAL + 4,), torch.int32)
        return N.lib().s3grl_cn_fill(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), len(INDICES), N.ptr(links), 3, 1,
                                     N.ptr(cn_ptr), CN_TOTAL, N.ptr(out)), [out]

    yield call, "s3grl_cn_fill", "ncn: a link endpoint outside [0, N)"


@contextmanager
def _sketch_entry(masked):
    from s3grl_amd import _native as N
    from s3grl_amd import sketch as S

    eng = _engine()
    ip, ix = _graph()
    mh = torch.zeros((HOPS + 1, N_NODES, P), dtype=torch.int32, device=eng.device)
    hl = torch.zeros((HOPS + 1, N_NODES, 1 << HLL_P), dtype=torch.uint8, device=eng.device)
    N.check(N.lib().s3grl_sketch_build(eng._ctx, N_NODES, N.ptr(ip), N.ptr(ix), len(INDICES), HOPS, P, HLL_P, 0,
                                       N.ptr(mh), N.ptr(hl)), "s3grl_sketch_build")
    _, c, lc = S.hll_constants(HLL_P)
    lc = torch.as_tensor(lc).to(eng.device)
    K1 = HOPS + 1

    def call(links):
        outs = [_sentinel((3, K1, K1), torch.int32), _sentinel((3, K1, K1), torch.int64),
                _sentinel((3, K1, K1), torch.int32), _sentinel((3, K1, K1), torch.float32),
                _sentinel((3, HOPS * HOPS + 2 * HOPS), torch.float32)]
        ptrs = [N.ptr(o) for o in outs]
        if masked:
            return N.lib().s3grl_masked_sketch_pairs(eng._ctx, N_NODES, N.ptr(ip), N.ptr(ix), len(INDICES), HOPS, P,
                                                     HLL_P, N.ptr(mh), N.ptr(hl), N.ptr(lc), c, N.ptr(links), 3,
                                                     *ptrs), outs
        return N.lib().s3grl_sketch_pairs(eng._ctx, N_NODES, HOPS, P, HLL_P, N.ptr(mh), N.ptr(hl), N.ptr(lc), c,
                                          N.ptr(links), 3, *ptrs), outs

    yield (call, "s3grl_masked_sketch_pairs" if masked else "s3grl_sketch_pairs",
           "sketch: a link endpoint outside [0, N)")


@contextmanager
def _mf_score_entry():
    from s3grl_amd import _native as N
    from s3grl_amd.mf import MFTrainer

    t = MFTrainer(N_NODES, hidden=8, num_layers=2, dropout=0.0, lr=0.01, seed=0)
    try:
        def call(pairs):
            out = _sentinel((3,), torch.float32)
            return N.lib().s3grl_mf_score(t._h, N.ptr(pairs), 3, N.ptr(out)), [out]

        yield call, "s3grl_mf_score", "mf score: a node outside [0, N)"
    finally:
        t.close()


@contextmanager
def _linkclf_predict_entry():
    from s3grl_amd import _native as N
    from s3grl_amd.linkclf import LinkClassifier

    clf = LinkClassifier(DIM)
    emb = torch.ones((N_NODES, DIM), dtype=torch.float32, device=_engine().device)
    try:
        def call(pairs):
            outs = [_sentinel((3,), torch.uint8), _sentinel((3,), torch.float32)]
            return N.lib().s3grl_linkclf_predict(clf._h, N.ptr(emb), N_NODES, N.ptr(pairs), 3, None, N.ptr(outs[0]),
                                                 N.ptr(outs[1]), None), outs

        yield call, "s3grl_linkclf_predict", "linkclf predict: a node outside [0, N)"
    finally:
        clf.close()


ID_ENTRIES = {
    "heuristics_pairs cn": lambda: _pairs_entry(0),
    "heuristics_pairs aa": lambda: _pairs_entry(1),
    "heuristics_pairs ra": lambda: _pairs_entry(2),
    "heuristics_pairs jaccard": lambda: _pairs_entry(3),
    "heuristics_pairs pa": lambda: _pairs_entry(4),
    "heuristics_katz": _katz_entry,
    "cn_count": _cn_count_entry,
    "cn_fill": _cn_fill_entry,
    "sketch_pairs": lambda: _sketch_entry(False),
    "masked_sketch_pairs": lambda: _sketch_entry(True),
    "mf_score": _mf_score_entry,
    "linkclf_predict": _linkclf_predict_entry,
}


@pytest.mark.parametrize("entry", sorted(ID_ENTRIES))
def test_a_bad_id_is_refused_outputs_stay_and_the_next_call_succeeds(entry):
    from s3grl_amd import _native as N

    with ID_ENTRIES[entry]() as (call, what, text):
        good = _dev(LINKS, torch.int32)
        for bad in (N_NODES, -1):
            for place, at in PLACES.items():
                ids = np.asarray(LINKS, dtype=np.int32).reshape(-1).copy()
                ids[at] = bad
                status, outs = call(_dev(ids.reshape(2, 3), torch.int32))
                torch.cuda.synchronize()
                _refused(status, f"{what}, {bad} in the {place}", text)
                assert all(_untouched(o) for o in outs), (entry, bad, place)
                status, outs = call(good)
                torch.cuda.synchronize()
                N.check(status, f"{what} after a refusal")
                assert not any(_untouched(o) for o in outs), (entry, bad, place)


# ---- CSR checks -----------------------------------------------------------------------------------------------------

def _create_heuristics(ip, ix, nnz):
    from s3grl_amd import _native as N

    h = C.c_void_p()
    status = N.lib().s3grl_heuristics_create(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), None, nnz, C.byref(h))
    if status == N.OK:
        N.lib().s3grl_heuristics_destroy(h)
    return status, []


def _create_skipgram(ip, ix, nnz):
    from s3grl_amd import _native as N

    cfg = N.SkipgramCfg(DIM, 4, 2, 1, 1, 0, 1.0, 1.0)
    h = C.c_void_p()
    status = N.lib().s3grl_skipgram_create(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), nnz, C.byref(cfg), None,
                                           C.byref(h))
    if status == N.OK:
        N.lib().s3grl_skipgram_destroy(h)
    return status, []


def _build_sketch(ip, ix, nnz):
    from s3grl_amd import _native as N

    outs = [_sentinel((HOPS + 1, N_NODES, P), torch.int32), _sentinel((HOPS + 1, N_NODES, 1 << HLL_P), torch.uint8)]
    status = N.lib().s3grl_sketch_build(_engine()._ctx, N_NODES, N.ptr(ip), N.ptr(ix), nnz, HOPS, P, HLL_P, 0,
                                        N.ptr(outs[0]), N.ptr(outs[1]))
    return status, outs


CSR_ENTRIES = {
    "heuristics_create": (_create_heuristics, "heuristics: malformed CSR (indptr not monotone from 0 to nnz, a column "
                          "outside [0, N), or a row not strictly ascending)"),
    "skipgram_create": (_create_skipgram, "node2vec: malformed CSR (indptr not monotone from 0 to nnz, or a column "
                        "outside [0, N))"),
    "sketch_build": (_build_sketch, "sketch: malformed CSR (indptr not monotone from 0 to nnz, or a column outside "
                     "[0, N))"),
}


def _with(values, at, value):
    out = list(values)
    out[at] = value
    return out


BROKEN = {    # (indptr, indices): refused by all three
    "indptr[0] = 1": (_with(INDPTR, 0, 1), INDICES),
    "a decreasing step in indptr": ([0, 3, 1, 5, 6], INDICES),
    "indptr[N] = nnz - 1": (_with(INDPTR, N_NODES, len(INDICES) - 1), INDICES),
    "a column equal to N": (INDPTR, _with(INDICES, 2, N_NODES)),
    "a column equal to -1": (INDPTR, _with(INDICES, 5, -1)),
}
UNSORTED = {  # refused by heuristics, accepted by the other two
    "a descending row": (INDPTR, [1, 2, 0, 1, 3, 2]),
    "a duplicate column": (INDPTR, [1, 0, 0, 1, 3, 2]),
}


@pytest.mark.parametrize("fault", sorted(BROKEN) + sorted(UNSORTED))
@pytest.mark.parametrize("entry", sorted(CSR_ENTRIES))
def test_a_broken_csr_is_refused_and_the_next_call_succeeds(entry, fault):
    from s3grl_amd import _native as N

    call, text = CSR_ENTRIES[entry]
    indptr, indices = BROKEN[fault] if fault in BROKEN else UNSORTED[fault]
    status, outs = call(_dev(indptr, torch.int64), _dev(indices, torch.int32), len(INDICES))
    torch.cuda.synchronize()
    if fault in BROKEN or entry == "heuristics_create":
        _refused(status, f"{entry}, {fault}", text)
        assert all(_untouched(o) for o in outs), (entry, fault)
    else:
        N.check(status, f"{entry}, {fault}")
    status, _ = call(*_graph(), len(INDICES))
    torch.cuda.synchronize()
    N.check(status, f"{entry} after {fault}")


@pytest.mark.parametrize("entry", sorted(CSR_ENTRIES))
def test_a_graph_without_entries_is_accepted(entry):
    from s3grl_amd import _native as N

    status, _ = CSR_ENTRIES[entry][0](_dev([0] * (N_NODES + 1), torch.int64), _dev([], torch.int32), 0)
    torch.cuda.synchronize()
    N.check(status, f"{entry}, nnz = 0")
