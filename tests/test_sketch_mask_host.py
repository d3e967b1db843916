"""CPU checks of the masked-sketch restatement (tests/sketch_mask_reference.py): the closed form on
the unmasked tables against the definition (one rebuild of the sketches per link on the graph without that link),
byte for byte, on every kind of link; what masking leaves alone; the named faults against that byte equality; the
refusals that need no device; and the public surface of `s3grl_masked_sketch_pairs`."""
import inspect
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import sketch_mask_cases as MC
import sketch_mask_reference as MR
import sketch_reference as R

REPO = Path(__file__).resolve().parent.parent
P, HLL_P = 128, 8


def _differ(a, b):
    return int(np.count_nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)))


@lru_cache(maxsize=None)
def _closed(name, hops, fault=None):
    A, links = MC.every_case()[name]
    mh, hl = R.sketches(A, hops, P, HLL_P, seed=0)
    return MR.masked_link_outputs(A, mh, hl, links, HLL_P, fault)


@lru_cache(maxsize=None)
def _rebuilt(name, hops):
    A, links = MC.every_case()[name]
    return MR.rebuilt_link_outputs(A, links, hops, P, HLL_P, seed=0)


@lru_cache(maxsize=None)
def _unmasked(name, hops):
    A, links = MC.every_case()[name]
    mh, hl = R.sketches(A, hops, P, HLL_P, seed=0)
    return R.link_outputs(mh, hl, links, HLL_P)


# ---- the cases hold what they say ---------------------------------------------------------------------------------

def test_the_cases_hold_every_kind_of_link():
    A, links = MC.directed_case()
    st = MC.stored(A, links)
    kinds = {(bool(a), bool(b)) for a, b in st.T}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    deg = np.diff(A.indptr)
    u, v = links
    assert ((u == v) & (A[u, v].A1 != 0)).any() and ((u == v) & (A[u, v].A1 == 0)).any()      # u == v, both ways
    loops = A.diagonal() != 0
    assert ((u != v) & loops[u] & st[0]).any()                                              # an endpoint's self-loop
    assert ((deg[u] == 1) & st[0]).any()                                                    # its only key: the partner
    assert deg[14] == 0 and A[:, 14].nnz == 0 and (u == 14).any()                           # isolated
    A, links = MC.length_case()
    st = MC.stored(A, links)
    masked = np.r_[np.diff(A.indptr)[links[0]][st[0]], np.diff(A.indptr)[links[1]][st[1]]]
    assert set(MC.LENGTHS) - {0} <= set(masked.tolist()) and (np.diff(A.indptr)[links[0]] == 0).any()
    A, links = MC.long_case()
    st, deg = MC.stored(A, links), np.diff(A.indptr)
    long_u, long_v = deg[links[0]] > MC.SPLIT_KEYS, deg[links[1]] > MC.SPLIT_KEYS
    assert (st[0] & st[1] & long_u & long_v).any() and (st[0] & st[1] & long_u & ~long_v).any()
    assert (~st[0] & ~st[1] & long_u).any()
    assert MC.quarter_positions(600) == [0, 75, 149, 150, 225, 299, 300, 375, 449, 450, 525, 599]
    assert MC.random_case()[1].shape[1] <= 32


# ---- the closed form is the definition ------------------------------------------------------------------------------

@pytest.mark.parametrize("hops", (1, 2))
@pytest.mark.parametrize("name", ("random", "directed", "lengths", "hub", "long"))
def test_closed_form_equals_a_rebuild_per_link(name, hops):
    closed, rebuilt = _closed(name, hops), _rebuilt(name, hops)
    for k in MR.NAMES:
        differ = _differ(closed[k], rebuilt[k])
        print(f"[mask] {name} hops {hops} {k}: {differ} bytes differ from the rebuild")
        assert closed[k].dtype == rebuilt[k].dtype and closed[k].shape == rebuilt[k].shape and differ == 0, k


@pytest.mark.parametrize("hops", (1, 2))
def test_links_that_are_no_entry_keep_the_unmasked_outputs_and_most_entries_change(hops):
    stored_links = changed = 0
    for name, (A, links) in MC.every_case().items():
        closed, plain = _closed(name, hops), _unmasked(name, hops)
        st = MC.stored(A, links).any(axis=0)
        for k in MR.NAMES:
            assert _differ(closed[k][~st], plain[k][~st]) == 0, (name, k)
        rows = (closed["features"][st].view(np.uint32) != plain["features"][st].view(np.uint32)).any(axis=1)
        stored_links, changed = stored_links + int(st.sum()), changed + int(rows.sum())
    print(f"[mask] hops {hops}: {changed} of {stored_links} stored links change their features under masking")
    assert 2 * changed >= stored_links > 0


@pytest.mark.parametrize("hops", (1, 2))
def test_the_reversed_link_gives_the_transposes(hops):
    for name, (A, links) in MC.every_case().items():
        mh, hl = R.sketches(A, hops, P, HLL_P, seed=0)
        fwd = _closed(name, hops)
        rev = MR.masked_link_outputs(A, mh, hl, links[::-1].copy(), HLL_P)
        for k in ("match", "T", "z", "intersections"):
            assert _differ(rev[k], np.ascontiguousarray(fwd[k].transpose(0, 2, 1))) == 0, (name, k)
        # (the features swap their two subtractions under the reversal, so they transpose only up to an fp64 ulp)


# ---- the named faults leave the byte equality ---------------------------------------------------------------------

@pytest.mark.parametrize("fault,hops", (("partner_kept_hop1", 1), ("partner_kept_hop1", 2), ("partner_kept_hop2", 2),
                                        ("own_hop1_left_out", 2)))
def test_named_faults_break_byte_equality(fault, hops):
    assert fault in MR.FAULTS
    differ = {k: 0 for k in MR.NAMES}
    for name in MC.every_case():
        good, bad = _rebuilt(name, hops), _closed(name, hops, fault)
        for k in MR.NAMES:
            differ[k] += _differ(good[k], bad[k])
    print(f"[mask] {fault} hops {hops}: bytes that differ {differ}")
    assert differ["match"] and differ["features"] and differ["intersections"]


# ---- refusals that need no device -----------------------------------------------------------------------------------

def test_mask_refusals_without_a_device():
    from s3grl_amd import sketch as S

    for method in (S.SketchGraph.features, S.SketchGraph.intersections, S.SketchGraph.raw):
        assert inspect.signature(method).parameters["mask"].default is False
    assert inspect.signature(S.run_buddy).parameters["mask"].default is False
    S.check_mask(1), S.check_mask(2)
    for hops in (3, 4):
        with pytest.raises(NotImplementedError, match="hops <= 2"):
            S.check_mask(hops)
        with pytest.raises(NotImplementedError, match="hops <= 2"):
            S.run_buddy(None, hops=hops, mask=True)
    with pytest.raises(ValueError, match="structure"):
        S.run_buddy(None, mask=True, structure=lambda links: links)
    with pytest.raises(ValueError):
        S.run_buddy(None, hops=5, mask=True)                     # the envelope comes first
    links = np.array([[0], [1]])
    shell = object.__new__(S.SketchGraph)                        # closed: that is said first, as without mask
    shell.num_nodes, shell.hops, shell.minhash = 3, 3, None
    for method in (shell.features, shell.intersections, shell.raw):
        with pytest.raises(RuntimeError, match="closed"):
            method(links, mask=True)
    shell.minhash = object()                                     # open at hops 3: refused before ids, engine or GPU
    for method in (shell.features, shell.intersections, shell.raw):
        with pytest.raises(NotImplementedError, match="hops <= 2"):
            method(links, mask=True)
    with pytest.raises(NotImplementedError):
        MR.masked_rows(np.zeros(2, np.int64), np.zeros(0, np.int64), np.zeros((4, 1, 64), np.uint32),
                       np.zeros((4, 1, 128), np.uint8), 0, 0)


# ---- the public surface: fails without the feature ----------------------------------------------------------------

def test_masked_call_is_declared_exported_and_refuses_through_the_abi():
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    assert len(re.findall(r"\bs3grl_masked_sketch_pairs\s*\(", header)) == 1
    assert "s3grl_masked_sketch_pairs" in _native.SYMBOLS
    assert re.search(r"#define\s+S3GRL_ABI_VERSION\s+6\b", header) and _native.ABI_VERSION == 6
    lib = _native.lib()
    call = lib.s3grl_masked_sketch_pairs
    assert call is not None and lib.s3grl_abi_version() == 6

    def refused(num_nodes=3, num_entries=0, hops=2, num_perm=128, hll_p=8, num_links=0):
        return call(None, num_nodes, None, None, num_entries, hops, num_perm, hll_p, None, None, None, 1.0, None,
                    num_links, None, None, None, None, None)

    assert refused() == _native.ERR_INVALID_ARGUMENT             # null context and tables
    for hops in (3, 4):
        assert refused(hops=hops) == _native.ERR_NOT_IMPLEMENTED
        assert "hops <= 2" in lib.s3grl_last_error().decode()
    for bad in (dict(hops=0), dict(hops=5), dict(num_perm=100), dict(hll_p=6), dict(hll_p=11), dict(num_nodes=0),
                dict(num_nodes=(1 << 24) + 1), dict(num_entries=-1), dict(num_entries=1 << 31), dict(num_links=-1),
                dict(num_links=1 << 31), dict(hops=5, num_links=-1)):
        assert refused(**bad) == _native.ERR_INVALID_ARGUMENT, bad
