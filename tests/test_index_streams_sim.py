"""clx_index_streams_device's kernels and host steps (clx_index.hip, unmodified) under the wave simulator against the host indexer run
on each stream alone: the whole shard of index_cases.py, the same shard shuffled (no answer depends on a stream's neighbours), the
arena flush against an inaccessible page, every refused argument, and the capacity protocol."""
import numpy as np
import pytest

import claxon_amd as cx
import index_cases as ic
import simlib_index as si


@pytest.fixture(scope="module")
def cases():
    c = ic.streams()
    a = ic.host_answers(c)
    ic.check_shape(c, a)
    return c, a


def test_whole_shard_equals_host_indexer_per_stream(cases):
    c, a = cases
    arena, offs, lens, starts, order = ic.shard(c)
    got = si.index_streams(arena, offs, lens, starts)
    ic.assert_equal(got, ic.expected(c, a, offs, order), "shard")
    assert int(got[2][-1]) == got[0].size >= 300


def test_shuffled_shard(cases):
    c, a = cases
    order = np.random.default_rng(4).permutation(len(c)).tolist()
    assert order != sorted(order)
    arena, offs, lens, starts, order = ic.shard(c, order)
    got = si.index_streams(arena, offs, lens, starts)
    ic.assert_equal(got, ic.expected(c, a, offs, order), "shuffled")


def test_arena_flush_against_an_inaccessible_page(cases):
    """The padded end of the arena (round16(len) + 32 bytes, all 0xff behind the last stream) is followed by a page that faults."""
    c, a = cases
    whole = list(range(len(c)))
    for order in (whole, whole[::-1]):
        arena, offs, lens, starts, order = ic.shard(c, order)
        got = si.index_streams(arena, offs, lens, starts, guarded=True)
        ic.assert_equal(got, ic.expected(c, a, offs, order), "guarded")
    # a stream that ends in the middle of a header, flush against the arena's end
    k = [n for n, _, _ in c].index("twice_a")
    d = c[k][1][:int(a[k][0]["byte_off"][3]) + 3]
    got = si.index_streams(d, [0], [d.size], [0], guarded=True)
    want = cx.index_frames(d, 0)
    assert got[0].tobytes() == want[0].tobytes() and int(got[3][0]) == want[2] and got[0].size == 2


def _raw(arena, offs, lens, starts, cap=64, descs=True, first=True, stops=True, found=True):
    al = si.aligned(np.ascontiguousarray(arena, dtype=np.uint8))
    offs = np.array(offs, dtype=np.uint64); lens = np.array(lens, dtype=np.uint64)
    starts = None if starts is None else np.array(starts, dtype=np.uint64)
    d = np.zeros(max(cap, 1), dtype=cx.FRAME_DESC_DTYPE); h = np.zeros(max(cap, 1), dtype=cx.FRAME_HEADER_DTYPE)
    f = np.zeros(offs.size + 1, dtype=np.uint64); s = np.zeros(max(offs.size, 1), dtype=np.uint64)
    return si.index_streams_raw(al.ctypes.data, len(arena), offs.ctypes.data, lens.ctypes.data, None if starts is None else starts.ctypes.data,
                                offs.size, d.ctypes.data if descs else None, h.ctypes.data, cap, f.ctypes.data if first else None,
                                s.ctypes.data if stops else None, null_found=not found)


def test_argument_errors():
    arena = np.zeros(256, dtype=np.uint8)
    for offs, lens, starts, stream, word in (
            ([0, 40], [32, 16], None, 1, "multiple of 16"),
            ([32, 0], [16, 16], None, 1, "ascend"),
            ([0, 16], [32, 16], None, 1, "overlap"),
            ([0, 240], [16, 32], None, 1, "outside"),
            ([0, 512], [16, 0], None, 1, "outside"),
            ([0, 16, 32], [16, 16, 16], [0, 0, 17], 2, "start")):
        st, _, err = _raw(arena, offs, lens, starts)
        assert st == cx.API_ERROR and "stream %d" % stream in err and word in err, (offs, err)
    for kw in (dict(descs=False), dict(first=False), dict(stops=False), dict(found=False)):
        st, _, err = _raw(arena, [0], [16], None, **kw)
        assert st == cx.API_ERROR and "null" in err, (kw, err)
    st, found, _ = _raw(arena, [0, 16], [16, 0], [16, 0])       # starts == lens is allowed: nothing to index
    assert st == cx.OK and found == 0


def test_empty_input():
    arena = np.zeros(64, dtype=np.uint8)
    d, h, first, stops = si.index_streams(arena, [], [])
    assert d.size == 0 and first.tolist() == [0] and stops.size == 0
    d, h, first, stops = si.index_streams(arena, [0, 0, 16], [0, 0, 0], [0, 0, 0])
    assert d.size == 0 and first.tolist() == [0, 0, 0, 0] and stops.tolist() == [0, 0, 16]
    d, h, first, stops = si.index_streams(arena[:0], [0], [0])
    assert d.size == 0 and first.tolist() == [0, 0]


def test_undersized_cap_reports_the_count_then_succeeds(cases):
    c, a = cases
    names = [n for n, _, _ in c]
    order = [names.index(n) for n in ("short.flac", "md5_16_2", "cut_head", "len0", "md5_24_1")]
    arena, offs, lens, starts, order = ic.shard(c, order)
    want = ic.expected(c, a, offs, order)
    need = want[0].size
    assert need == 1 + 6 + 9 + 0 + 7
    for cap in (0, need - 1):
        with pytest.raises(cx.ClaxonError) as e:
            si.index_streams(arena, offs, lens, starts, cap=cap)
        assert e.value.status == cx.API_ERROR and e.value.n_found == need and "do not fit" in e.value.message
    ic.assert_equal(si.index_streams(arena, offs, lens, starts, cap=need), want, "second call")
