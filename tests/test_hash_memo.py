"""The Allocate -> PreStart hash memo of _fastwire (native/hashmemo.h, "hash
memo"): Allocate's digest leaves runs fragment -> hash, PreStart's digest takes
it instead of hashing again. Every result is checked against
types.hash_device_ids and against the same call with the memo off."""
import random
import threading

import pytest

from elastic_gpu_agent_amd.types import hash_device_ids

_fastwire = pytest.importorskip("elastic_gpu_agent_amd._fastwire")


def ids_range(start, n, gpu=0):
    return [f"{gpu}-{i:06d}" for i in range(start, start + n)]


def alloc_req(*containers):
    return _fastwire.encode_nested_string_lists([list(c) for c in containers])


def prestart_req(ids, seed=None):
    ids = list(ids)
    if seed is not None:
        random.Random(seed).shuffle(ids)
    return _fastwire.encode_string_list(ids)


@pytest.fixture
def memo():
    """A fresh memo at the default cap; the default is restored afterwards."""
    _fastwire.hash_memo_configure(0)
    _fastwire.hash_memo_configure(_fastwire.HASH_MEMO_ENTRIES)
    base = _fastwire.hash_memo_stats()

    def delta():
        now = _fastwire.hash_memo_stats()
        return {k: now[k] - base[k] for k in ("puts", "hits", "misses", "evictions")}

    yield delta
    _fastwire.hash_memo_configure(0)
    _fastwire.hash_memo_configure(_fastwire.HASH_MEMO_ENTRIES)


def with_memo_off(fn, *args):
    cap = _fastwire.hash_memo_stats()["cap"]
    entries = _fastwire.hash_memo_stats()["entries"]
    assert entries == 0, "turning the memo off here would drop entries"
    _fastwire.hash_memo_configure(0)
    try:
        return fn(*args)
    finally:
        _fastwire.hash_memo_configure(cap)


def check_prestart(req, ids):
    """decode_prestart_digest3 with the memo as it is == with the memo off ==
    the Python hash."""
    got = _fastwire.decode_prestart_digest3(req)
    assert got[0] == hash_device_ids(sorted(ids))
    assert got[1] == len(ids)
    assert got == with_memo_off(_fastwire.decode_prestart_digest3, req)
    return got


def test_defaults():
    assert _fastwire.HASH_MEMO_ENTRIES == 256
    assert _fastwire.HASH_MEMO_MAX_KEY == 4096
    assert _fastwire.hash_memo_stats()["cap"] == 256


def test_smallest_set_that_qualifies(memo):
    ids = ids_range(0, 1024)
    assert _fastwire.digest_allocate_request(alloc_req(ids)) == [
        (hash_device_ids(ids), 1024)]
    assert memo()["puts"] == 1
    got = check_prestart(prestart_req(ids), ids)
    assert got[3] is True
    assert memo()["hits"] == 1 and memo()["misses"] == 0


def test_1023_ids_make_no_put(memo):
    ids = ids_range(0, 1023)
    assert _fastwire.digest_allocate_request(alloc_req(ids)) == [
        (hash_device_ids(ids), 1023)]
    assert memo()["puts"] == 0
    got = check_prestart(prestart_req(ids), ids)
    assert got[3] is False
    assert memo()["hits"] == 0


def test_sorted_allocate_then_shuffled_prestart_hits_once(memo):
    ids = ids_range(100, 18432)
    want = hash_device_ids(ids)
    assert _fastwire.digest_allocate_request(alloc_req(ids)) == [(want, len(ids))]
    first = _fastwire.decode_prestart_digest3(prestart_req(ids, seed=1))
    assert first == (want, len(ids), b'[["0-",6,100,18432]]', True)
    assert memo() == {"puts": 1, "hits": 1, "misses": 0, "evictions": 0}
    # the hit consumed the entry: the same PreStart again hashes
    second = _fastwire.decode_prestart_digest3(prestart_req(ids, seed=2))
    assert second == first
    assert memo() == {"puts": 1, "hits": 1, "misses": 1, "evictions": 0}
    assert first == with_memo_off(_fastwire.decode_prestart_digest3, prestart_req(ids, seed=1))


def test_shuffled_allocate_then_sorted_prestart_hits(memo):
    ids = ids_range(0, 4096)
    shuffled = list(ids)
    random.Random(3).shuffle(shuffled)
    assert _fastwire.digest_allocate_request(alloc_req(shuffled)) == [
        (hash_device_ids(ids), 4096)]
    assert _fastwire.decode_prestart_digest3(prestart_req(ids))[0] == hash_device_ids(ids)
    assert memo()["hits"] == 1


def test_set_that_differs_by_one_gap_misses(memo):
    ids = ids_range(0, 2048)
    other = ids[:1000] + ids[1001:] + ids_range(2048, 1)  # same count, one gap
    assert len(other) == len(ids)
    req_other = prestart_req(other, seed=4)
    off = with_memo_off(_fastwire.decode_prestart_digest3, req_other)
    _fastwire.digest_allocate_request(alloc_req(ids))
    got = _fastwire.decode_prestart_digest3(req_other)
    assert got == off
    assert got[0] == hash_device_ids(sorted(other)) != hash_device_ids(ids)
    assert got[3] is True
    assert memo()["hits"] == 0 and memo()["misses"] == 1
    # the entry of the first set is still there for its own PreStart
    assert _fastwire.decode_prestart_digest3(prestart_req(ids, seed=5))[0] == \
        hash_device_ids(ids)
    assert memo()["hits"] == 1


def test_two_container_allocate(memo):
    a, b = ids_range(0, 2048), ids_range(0, 1500, gpu=1)
    small = ids_range(5000, 10)
    req = alloc_req(a, small, b)
    want = [(hash_device_ids(a), 2048), (hash_device_ids(small), 10),
            (hash_device_ids(b), 1500)]
    assert with_memo_off(_fastwire.digest_allocate_request, req) == want
    assert memo()["puts"] == 0
    assert _fastwire.digest_allocate_request(req) == want
    assert memo()["puts"] == 2  # the 10-ID container is too small to try
    got_b = _fastwire.decode_prestart_digest3(prestart_req(b, seed=6))
    got_a = _fastwire.decode_prestart_digest3(prestart_req(a, seed=7))
    assert (got_a[0], got_b[0]) == (want[0][0], want[2][0])
    assert memo()["hits"] == 2 and memo()["misses"] == 0
    assert got_a == with_memo_off(_fastwire.decode_prestart_digest3, prestart_req(a, seed=7))


def test_eviction_drops_the_oldest(memo):
    _fastwire.hash_memo_configure(2)
    sets = [ids_range(10000 * k, 1024) for k in range(3)]
    for s in sets:
        _fastwire.digest_allocate_request(alloc_req(s))
    st = _fastwire.hash_memo_stats()
    assert st["entries"] == 2 and memo()["evictions"] == 1
    for s in sets:  # the first was evicted: a miss with the right hash
        assert _fastwire.decode_prestart_digest3(prestart_req(s, seed=8))[0] == \
            hash_device_ids(s)
    assert memo()["hits"] == 2 and memo()["misses"] == 1
    assert _fastwire.hash_memo_stats()["entries"] == 0


def test_key_over_the_length_cap_is_not_stored(memo):
    # 300 runs of 8 IDs: qualifies (runs <= n / 8), fragment > 4 KiB
    ids = [i for k in range(300) for i in ids_range(10 * k, 8)]
    _fastwire.digest_allocate_request(alloc_req(ids))
    got = check_prestart(prestart_req(ids, seed=9), ids)
    assert got[3] is True and len(got[2]) > _fastwire.HASH_MEMO_MAX_KEY
    assert memo()["puts"] == 0 and memo()["hits"] == 0
    assert _fastwire.hash_memo_stats()["entries"] == 0


def test_configure_zero_turns_it_off_and_empties_it(memo):
    ids = ids_range(0, 1024)
    _fastwire.digest_allocate_request(alloc_req(ids))
    assert _fastwire.hash_memo_stats()["entries"] == 1
    _fastwire.hash_memo_configure(0)
    assert _fastwire.hash_memo_stats()["entries"] == 0
    before = _fastwire.hash_memo_stats()
    assert _fastwire.digest_allocate_request(alloc_req(ids)) == [
        (hash_device_ids(ids), 1024)]
    got = _fastwire.decode_prestart_digest3(prestart_req(ids, seed=10))
    assert got == (hash_device_ids(ids), 1024, b'[["0-",6,0,1024]]', True)
    assert _fastwire.hash_memo_stats() == before  # no put, no hit, no miss
    with pytest.raises(Exception):
        _fastwire.hash_memo_configure(-1)


def test_threads_on_distinct_sets(memo):
    errors = []

    def worker(t):
        try:
            for k in range(25):
                ids = ids_range(100000 * t + 2000 * k, 1024 + k, gpu=t)
                want = hash_device_ids(ids)
                assert _fastwire.digest_allocate_request(alloc_req(ids)) == [
                    (want, len(ids))]
                got = _fastwire.decode_prestart_digest3(prestart_req(ids, seed=k))
                assert got[0] == want and got[1] == len(ids) and got[3] is True
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert memo() == {"puts": 100, "hits": 100, "misses": 0, "evictions": 0}
