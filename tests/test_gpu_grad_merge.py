"""`scone_grad_merge_map` / `scone_grad_merge_rows` (`SconeTable.grad_merge_map`, `.grad_merge_rows`, `.grad_merge`) against the
numpy statement tests/grad_merge_fixture.py: ids and maps equal, rows bit for bit (a NaN matches any NaN).

The map is always called through the C ABI on buffers that end in canary words, so "nothing is written outside the stated
capacities" is checked in every case, and entries of d_src_a / d_src_b behind n_out must read "absent".
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_merge_fixture as GM  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 257)
WIDTHS = (4, 252, 256, 260, 768, 4104)
CANARY = 16
CANARY_WORD = 0x5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _table(d, n=8):
    from scone_amd.hip_backend import SconeTable
    return SconeTable(3, n, dim=d, table_format="fp32")


def _canaried(n, dtype):
    t = torch.full((n + CANARY,), CANARY_WORD, dtype=dtype, device="cuda")
    return t


def _intact(t, n):
    return bool((t[n:] == CANARY_WORD).all())


def _raw_map(table, a, b, sync=True):
    """The C call on canaried buffers.  Returns (rc, n_out, dict of whole numpy arrays incl. canaries, all canaries intact)."""
    from scone_amd import _lib as L
    a_t, b_t = torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(b, dtype=np.int64)).cuda()
    n_a, n_b = a_t.numel(), b_t.numel()
    cap = n_a + n_b
    bufs = {"ids": _canaried(cap, torch.int64), "src_a": _canaried(cap, torch.int32), "src_b": _canaried(cap, torch.int32),
            "pos_a": _canaried(n_a, torch.int32), "pos_b": _canaried(n_b, torch.int32), "n_out": _canaried(1, torch.int64)}
    need = L.grad_merge_scratch(n_a, n_b)
    scratch = torch.full((need + 4 * CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    h_n = C.c_uint64(0xDEAD)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().scone_grad_merge_map(table._h, p(a_t) if n_a else None, n_a, p(b_t) if n_b else None, n_b, p(bufs["ids"]),
                                      p(bufs["src_a"]), p(bufs["src_b"]), p(bufs["pos_a"]), p(bufs["pos_b"]), p(scratch),
                                      p(bufs["n_out"]), C.byref(h_n) if sync else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    caps = {"ids": cap, "src_a": cap, "src_b": cap, "pos_a": n_a, "pos_b": n_b, "n_out": 1}
    intact = all(_intact(bufs[k], caps[k]) for k in bufs) and bool((scratch[need:] == 0x5A).all())
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k in ("src_a", "src_b", "pos_a", "pos_b"):
        out[k] = out[k].view(np.uint32)
    return rc, int(h_n.value), out, intact, caps


def _check_map(table, a, b, tag):
    from scone_amd import _lib as L
    rc, n_out, got, intact, caps = _raw_map(table, a, b)
    assert rc == L.OK, tag
    assert intact, f"{tag}: a canary word behind an output buffer was written"
    ids, src_a, src_b, pos_a, pos_b = GM.merge_map(a, b)
    cap = caps["ids"]
    assert n_out == len(ids) == int(got["n_out"][0]), f"{tag}: n_out {n_out} / {int(got['n_out'][0])}, the fixture has {len(ids)}"
    assert np.array_equal(got["ids"][:n_out], ids), tag
    assert np.array_equal(got["src_a"][:n_out], src_a) and np.array_equal(got["src_b"][:n_out], src_b), tag
    assert (got["src_a"][n_out:cap] == GM.ABSENT).all() and (got["src_b"][n_out:cap] == GM.ABSENT).all(), f"{tag}: entries behind n_out"
    assert np.array_equal(got["pos_a"][:len(pos_a)], pos_a) and np.array_equal(got["pos_b"][:len(pos_b)], pos_b), tag
    assert table.status() == 0, tag


# ------------------------------------------------------------------ 1. the map: sizes x list relations
def _relation(rel, n_a, n_b, rng):
    """Two ascending lists of distinct ids, or None where the relation needs other sizes."""
    if rel == "disjoint":
        return 2 * np.arange(n_a) * 3, 2 * np.sort(rng.choice(4 * n_b + 1, n_b, replace=False)) * 3 + 1
    if rel == "identical":
        if n_a != n_b:
            return None
        a = np.sort(rng.choice(5 * n_a + 1, n_a, replace=False))
        return a, a.copy()
    if rel == "interleaved":
        span = max(n_a, n_b) * 2 + 1
        return np.sort(rng.choice(span, n_a, replace=False)), np.sort(rng.choice(span, n_b, replace=False))
    if rel == "subset":
        if n_b > n_a:
            return None
        a = np.sort(rng.choice(3 * n_a + 1, n_a, replace=False))
        return a, np.sort(rng.choice(a, n_b, replace=False))
    if rel == "a_below_b":
        return np.arange(n_a) * 2, 2 * n_a + 5 + np.arange(n_b) * 3
    if rel == "b_below_a":
        return 3 * n_b + 7 + np.arange(n_a) * 2, np.arange(n_b) * 3
    raise AssertionError(rel)


@pytest.mark.parametrize("rel", ["disjoint", "identical", "interleaved", "subset", "a_below_b", "b_below_a"])
def test_map_over_sizes_and_relations(rel):
    table = _table(8)
    rng = np.random.default_rng(len(rel))
    done = 0
    for n_a in SIZES:
        for n_b in SIZES:
            lists = _relation(rel, n_a, n_b, rng)
            if lists is None:
                continue
            _check_map(table, lists[0], lists[1], f"{rel}-{n_a}-{n_b}")
            done += 1
    assert done >= len(SIZES)


def test_map_with_ids_at_the_edges_of_32_bits_and_beyond():
    table = _table(8)
    edge = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, 1 << 40, (1 << 40) + 1, (1 << 62)]
    a = np.array([edge[i] for i in (0, 2, 4, 5, 7, 9)], dtype=np.int64)
    b = np.array([edge[i] for i in (0, 1, 3, 4, 6, 7, 8)], dtype=np.int64)
    _check_map(table, a, b, "edges")
    _check_map(table, b, a, "edges-swapped")
    # the order is SIGNED: a negative id (never a table row, but an int64) sorts first
    _check_map(table, np.array([-(1 << 40), -1, 5], dtype=np.int64), np.array([-1, 0, 1 << 40], dtype=np.int64), "signed")
    # more than one tile of flags and a tile boundary inside b
    rng = np.random.default_rng(9)
    a = np.sort(rng.choice(1 << 20, 3000, replace=False)) + (1 << 33)
    b = np.sort(np.concatenate([rng.choice(a, 1000, replace=False), (1 << 33) + (1 << 20) + np.arange(1049)]))
    assert len(b) == 2049 and GM.is_valid(b)
    _check_map(table, a, b, "tiles")


def test_unsynchronised_map_leaves_the_count_on_the_device():
    table = _table(8)
    a, b = np.arange(0, 100, 2), np.arange(0, 150, 3)
    rc, h_n, got, intact, _ = _raw_map(table, a, b, sync=False)
    assert rc == 0 and intact and h_n == 0xDEAD, "h_n_out == NULL: nothing is returned to the host"
    assert int(got["n_out"][0]) == len(np.union1d(a, b))
    m = table.grad_merge_map(torch.from_numpy(a), torch.from_numpy(b), sync=False)
    assert m.n_out is None and m.ids.numel() == len(a) + len(b) and int(m.d_n_out.item()) == len(np.union1d(a, b))


# ------------------------------------------------------------------ 2. the rows
def _rows_case(table, d, n_a, n_b, seed, edge=True):
    rng = np.random.default_rng(seed)
    span = max(n_a, n_b) * 2 + 1
    a, b = np.sort(rng.choice(span, n_a, replace=False)), np.sort(rng.choice(span, n_b, replace=False))
    make = GM.edge_rows if edge else (lambda n, d, s: np.random.default_rng(s).standard_normal((n, d)).astype(np.float32))
    return a.astype(np.int64), make(n_a, d, seed + 1), b.astype(np.int64), make(n_b, d, seed + 2)


def _gpu_merge(table, a, ra, b, rb):
    ids, rows = table.grad_merge(torch.from_numpy(a).cuda(), torch.from_numpy(ra).cuda(), torch.from_numpy(b).cuda(),
                                 torch.from_numpy(rb).cuda())
    return ids.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("d", WIDTHS)
def test_rows_at_every_width_with_edge_values(d):
    """d = 4: lane 0 only; 252 / 256 / 260: either side of one piece per lane; 768; 4104: five blocks and a ragged last one.
    Rows hold -0.0, subnormals, +-inf and NaN; the lists overlap in part, so all three kinds of output row occur."""
    table = _table(d)
    for n_a, n_b in ((65, 63), (0, 64), (257, 1), (1, 0), (0, 0)):
        a, ra, b, rb = _rows_case(table, d, n_a, n_b, seed=d + n_a)
        want_ids, want = GM.merge(a, ra, b, rb)
        if n_a == 65:
            _, src_a, src_b, _, _ = GM.merge_map(a, b)
            kinds = ((src_a != GM.ABSENT).astype(int) + 2 * (src_b != GM.ABSENT).astype(int))
            assert set(kinds.tolist()) == {1, 2, 3}
            assert np.signbit(want[want == 0]).any() and np.isnan(want).any() and np.isinf(want).any()
        ids, rows = _gpu_merge(table, a, ra, b, rb)
        assert np.array_equal(ids, want_ids) and rows.shape == want.shape
        assert GM.same_bits(rows, want), f"d={d} n_a={n_a} n_b={n_b}"
        again = _gpu_merge(table, a, ra, b, rb)[1]
        assert np.array_equal(again.view(np.uint32), rows.view(np.uint32)), "two runs differ"
    assert table.status() == 0


def test_copied_rows_keep_nan_payloads_and_negative_zero():
    d = 8
    table = _table(d)
    ra = np.array([[0x7FC01234, 0xFFC00001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FA00000]],
                  dtype=np.uint32).view(np.float32)
    rb = ra[:, ::-1].copy()
    ids, rows = _gpu_merge(table, np.array([3], dtype=np.int64), ra, np.array([9], dtype=np.int64), rb)
    assert ids.tolist() == [3, 9]
    assert np.array_equal(rows[0].view(np.uint32), ra[0].view(np.uint32)) and np.array_equal(rows[1].view(np.uint32), rb[0].view(np.uint32))


def test_one_workgroup_walks_300_output_rows(monkeypatch):
    """SCONE_OPT_MAX_BLOCKS=1 (read at create): four waves walk 300 output rows, each wave re-using itself."""
    d = 260
    monkeypatch.setenv("SCONE_OPT_MAX_BLOCKS", "1")
    table = _table(d)
    monkeypatch.delenv("SCONE_OPT_MAX_BLOCKS")
    a = np.arange(0, 400, 2, dtype=np.int64)                     # 200 rows
    b = np.arange(100, 400, dtype=np.int64)[:200]                # 200 rows, 100 of them a's
    ra, rb = GM.edge_rows(200, d, 1), GM.edge_rows(200, d, 2)
    want_ids, want = GM.merge(a, ra, b, rb)
    assert len(want_ids) == 300
    ids, rows = _gpu_merge(table, a, ra, b, rb)
    assert np.array_equal(ids, want_ids) and GM.same_bits(rows, want)
    free = _table(d)
    assert np.array_equal(_gpu_merge(free, a, ra, b, rb)[1].view(np.uint32), rows.view(np.uint32)), "the grid shows in the bits"


# ------------------------------------------------------------------ 3. outside the contract, and the refusals
@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_a_list_that_is_not_ascending_raises_bad_id_and_stays_in_bounds(which):
    from scone_amd import _lib as L
    table = _table(8)
    rng = np.random.default_rng(3)
    good = np.sort(rng.choice(500, 257, replace=False))
    bad = rng.integers(0, 300, size=65)                          # unsorted, with repeats
    assert not GM.is_valid(bad)
    a, b = {"a": (bad, good), "b": (good, bad), "both": (bad, bad[::-1].copy())}[which]
    rc, n_out, got, intact, caps = _raw_map(table, a, b)
    assert rc == L.OK and intact, "a canary word behind an output buffer was written"
    cap = len(a) + len(b)
    assert n_out <= cap
    for name, n in (("src_a", len(a)), ("src_b", len(b))):
        s = got[name][:cap]
        assert ((s == GM.ABSENT) | (s < n)).all(), f"{name} holds an index outside its list"
    assert (got["pos_a"][:len(a)] < cap).all() and (got["pos_b"][:len(b)] < cap).all()
    assert table.status() & L.ST_BAD_ID
    # a repeated id alone (ascending, not distinct) is outside the contract too
    rc, _, _, intact, _ = _raw_map(table, np.array([1, 2, 2, 3]), np.array([2, 5]))
    assert rc == L.OK and intact and table.status() & L.ST_BAD_ID
    _check_map(table, good, good[::2], "a valid call afterwards")


def test_refusals_write_nothing():
    from scone_amd import _lib as L
    from scone_amd.hip_backend import SconeTable
    table = _table(8)
    lib = L.lib()
    words = _canaried(64, torch.int64)
    p = C.c_void_p(words.data_ptr())
    h_n = C.c_uint64(7)
    stream = torch.cuda.current_stream().cuda_stream
    for n_a, n_b in (((1 << 32) - 2, 1), (1, (1 << 32) - 2), ((1 << 31), (1 << 31) - 1), ((1 << 32) - 1, 0)):
        assert n_a + n_b >= (1 << 32) - 1
        rc = lib.scone_grad_merge_map(table._h, p, n_a, p, n_b, p, p, p, p, p, p, p, C.byref(h_n), stream)
        assert rc == L.EINVAL and b"scone_grad_merge_map" in lib.scone_last_error(table._h)
    for args in ((None, 4, p, 4), (p, 4, None, 4)):             # a null list that is not empty
        rc = lib.scone_grad_merge_map(table._h, args[0], args[1], args[2], args[3], p, p, p, p, p, p, p, C.byref(h_n), stream)
        assert rc == L.EINVAL
    assert lib.scone_grad_merge_map(table._h, p, 4, p, 4, p, p, p, p, p, None, p, C.byref(h_n), stream) == L.EINVAL
    # rows: out == a, out == b
    rows = torch.full((16, 8), 3.0, dtype=torch.float32, device="cuda")
    other = torch.full((16, 8), 5.0, dtype=torch.float32, device="cuda")
    src = torch.arange(8, dtype=torch.int32, device="cuda")
    r, o, s = C.c_void_p(rows.data_ptr()), C.c_void_p(other.data_ptr()), C.c_void_p(src.data_ptr())
    assert lib.scone_grad_merge_rows(table._h, s, s, 8, r, o, r, stream) == L.EINVAL
    assert b"overlap" in lib.scone_last_error(table._h)
    assert lib.scone_grad_merge_rows(table._h, s, s, 8, o, r, r, stream) == L.EINVAL
    assert lib.scone_grad_merge_rows(table._h, s, s, (1 << 32) - 1, r, o, C.c_void_p(words.data_ptr()), stream) == L.EINVAL
    torch.cuda.synchronize()
    assert h_n.value == 7 and bool((words == CANARY_WORD).all()), "a refused call wrote"
    assert bool((rows == 3.0).all()) and bool((other == 5.0).all())
    no_table = SconeTable(3, 8, dim=0)
    assert lib.scone_grad_merge_map(no_table._h, p, 1, p, 1, p, p, p, p, p, p, p, C.byref(h_n), stream) == L.EINVAL
    assert lib.scone_grad_merge_rows(no_table._h, s, s, 8, r, o, C.c_void_p(words.data_ptr()), stream) == L.EINVAL
    with pytest.raises(ValueError):
        table.grad_merge(src.long(), rows[:8], src.long(), other[:8].half())
    assert table.status() == 0


# ------------------------------------------------------------------ 4. the glue it replaces
@pytest.mark.parametrize("d", [64, 768])
def test_grad_merge_equals_add_coalesced_on_finite_inputs(d):
    from scone_amd.training import _add_coalesced
    table = _table(d, n=600)
    for n_a, n_b in ((257, 65), (64, 64), (0, 63), (63, 0)):
        a, ra, b, rb = _rows_case(table, d, n_a, n_b, seed=7 * d + n_a, edge=False)
        ra[::3, ::5] = -0.0
        rb[::2, ::5] = -0.0
        ra[1::4, 1::7] = 1e-40
        ta, tra, tb, trb = (torch.from_numpy(x).cuda() for x in (a, ra, b, rb))
        old = torch.sparse_coo_tensor(ta[None], tra, (600, d), is_coalesced=True)
        glue = _add_coalesced(old, tb, trb)
        ids, rows = table.grad_merge(ta, tra, tb, trb)
        assert torch.equal(ids, glue._indices()[0])
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), glue._values().cpu().numpy().view(np.uint32)), (d, n_a, n_b)
