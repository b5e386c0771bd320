"""The fixed-stride run and the radix fallback of the device-set digest
(native/wirecore.h). A request whose IDs share one width is a run of entries
with the same two-byte header, which the walk handles at fixed stride; an
unsorted set of one width <= 8 is sorted as big-endian words. Every case goes
through all four _fastwire entry points and is compared with the Python
definitions: types.hash_device_ids / Device.new and json.dumps."""
import json
import random
import threading

import pytest

from elastic_gpu_agent_amd import _fastwire
from elastic_gpu_agent_amd.types import Device, hash_device_ids

MAX_STRIDE = 16  # kMaxStride in wirecore.h


# ---- hand-rolled wire encoding (independent of the codecs under test) -------

def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(field: int, payload: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def entry(i: str, field=1) -> bytes:
    return ld(field, i.encode())


def id_list(ids, field=1) -> bytes:
    return b"".join(entry(i, field) for i in ids)


# the unknown-field kinds of test_digest_fused.py's UNKNOWN, one by one
UNKNOWN_KINDS = [
    varint(2 << 3 | 0) + varint(300),
    varint(7 << 3 | 1) + b"\x01\x02\x03\x04\x05\x06\x07\x08",
    ld(9, b"0-zzz-not-an-id"),
    varint(4 << 3 | 5) + b"\xaa\xbb\xcc\xdd",
    varint(1 << 3 | 0) + varint(5),
]


def ref(ids):
    """(hash, count, sorted list, JSON fragment) by the Python definitions.
    The fragment keeps bytes >= 0x7f as they are (ensure_ascii=False); for
    plain ASCII IDs that is json.dumps' default output too."""
    d = Device.new(ids)
    assert d.hash == hash_device_ids(sorted(ids))
    return (d.hash, len(ids), list(d.list),
            json.dumps(list(d.list), separators=(",", ":"), ensure_ascii=False).encode())


def podresources_one(ids_body_field2: bytes) -> bytes:
    """one pod, one container, one ContainerDevices entry with this body"""
    c = ld(1, b"c") + ld(2, ld(1, b"res") + ids_body_field2)
    return ld(1, ld(1, b"pod") + ld(2, b"ns") + ld(3, c))


def check_body(ids, body, body2=None):
    """`body` is a field-1 encoding of `ids` (any extras included), `body2`
    the same in field 2; all four entry points must agree with Python"""
    h, n, sorted_ids, frag = ref(ids)
    assert _fastwire.digest_allocate_request(ld(1, body)) == [(h, n)]
    assert _fastwire.decode_prestart_digest(body) == (sorted_ids, h)
    h2, n2, frag2 = _fastwire.decode_prestart_digest2(body)
    assert (h2, n2) == (h, n)
    assert frag2 == frag
    assert json.loads(frag2) == sorted_ids
    if body2 is not None:
        rows = _fastwire.podresources_digest(podresources_one(body2))
        assert rows == ([("ns", "pod", "c", "res", h, n)] if ids else [])


def check(ids):
    check_body(ids, id_list(ids), id_list(ids, field=2))


def with_extra(ids, at, extra, field=1):
    """the entries of `ids` with raw bytes `extra` put in before entry `at`"""
    return id_list(ids[:at], field) + extra + id_list(ids[at:], field)


def fixed_ids(n, length, rng, alphabet="0123456789-"):
    return ["".join(rng.choice(alphabet) for _ in range(length)) for _ in range(n)]


# ---- run lengths and run boundaries ----------------------------------------

@pytest.mark.parametrize("length", range(1, MAX_STRIDE + 2))
def test_sorted_runs_of_every_length(length):
    """sizes 0, 1, 2 and a few hundred; the last entry of each ends exactly
    at the end of the buffer (for L < 8 a whole-word load would cross it)"""
    rng = random.Random(length)
    for n in (0, 1, 2, 3, 300):
        check(sorted(fixed_ids(n, length, rng)))


@pytest.mark.parametrize("length", [4, 8, 9, 12, 16])
def test_ids_that_differ_only_in_their_last_bytes(length):
    ids = ["0" * (length - 3) + f"{i:03d}" for i in range(200)]
    check(ids)
    for at in (0, 99, 198):
        bad = list(ids)
        bad[at], bad[at + 1] = bad[at + 1], bad[at]
        check(bad)


def test_runs_that_change_length_in_the_middle():
    ids = ([f"10-{i:04d}" for i in range(40)] + [f"9-{i:04d}" for i in range(40)]
           + [f"9-9{i:03d}-and-a-tail" for i in range(40)])
    assert ids == sorted(ids)
    check(ids)
    check(ids[::-1])
    check(["0-1", "0-10", "0-11", "0-2", "0-20"])
    check(["0-10", "0-11", "0-1"])


@pytest.mark.parametrize("kind", range(len(UNKNOWN_KINDS) + 1))
def test_run_broken_by_unknown_field(kind):
    extra = (UNKNOWN_KINDS + [b"".join(UNKNOWN_KINDS)])[kind]
    extra2 = extra  # none of these is a field-2 LEN entry either
    ids = sorted(fixed_ids(12, 6, random.Random(kind)))
    for at in range(len(ids) + 1):
        check_body(ids, with_extra(ids, at, extra), with_extra(ids, at, extra2, field=2))
    # after every entry: runs of one
    check_body(ids, b"".join(entry(i) + extra for i in ids),
               b"".join(entry(i, 2) + extra2 for i in ids))


def test_run_broken_by_two_byte_length():
    ids = sorted(fixed_ids(12, 6, random.Random(1)))
    for fill in ("!", "z"):          # sorts before / after the run's IDs
        long_id = fill * 130
        for at in range(len(ids) + 1):
            check_body(ids + [long_id], with_extra(ids, at, entry(long_id)),
                       with_extra(ids, at, entry(long_id, 2), field=2))


def test_run_broken_by_two_byte_tag():
    """0x8A 0x00 is field 1, LEN, written as a longer varint: same meaning,
    but only the generic reader takes it"""
    ids = sorted(fixed_ids(12, 6, random.Random(2)))
    for odd in ("0-0000", "zzzzzz", "5"):
        for at in range(len(ids) + 1):
            extra = b"\x8a\x00" + varint(len(odd)) + odd.encode()
            extra2 = b"\x92\x00" + varint(len(odd)) + odd.encode()
            check_body(ids + [odd], with_extra(ids, at, extra),
                       with_extra(ids, at, extra2, field=2))


def test_run_broken_by_empty_id():
    ids = sorted(fixed_ids(12, 6, random.Random(3)))
    for at in range(len(ids) + 1):
        check_body(ids + [""], with_extra(ids, at, entry("")),
                   with_extra(ids, at, entry("", 2), field=2))


@pytest.mark.parametrize("length", [1, 5, 8, 9, 16])
def test_duplicates_inside_a_run(length):
    base = sorted(set(fixed_ids(40, length, random.Random(length))))
    check([i for i in base for _ in range(3)])


@pytest.mark.parametrize("length", [2, 5, 8, 9, 16, 17])
def test_out_of_order_entry(length):
    """at the start, in the middle and as the last entry of a run"""
    ids = sorted(set(fixed_ids(60, length, random.Random(length))))
    assert len(ids) > 8
    for at in (0, len(ids) // 2, len(ids) - 2):
        bad = list(ids)
        bad[at], bad[at + 1] = bad[at + 1], bad[at]
        check(bad)
    check(ids[1:] + ids[:1])   # the smallest ID last
    check(ids[-1:] + ids[:-1])  # the largest ID first


# ---- escaping ---------------------------------------------------------------

SPECIALS = ['"', "\\", "\x00", "\x1f", "\x7f", "é", "€", " ", "!", "#", "[", "]"]


@pytest.mark.parametrize("length", [8, 3, 12, 16])
def test_escapes_at_every_offset(length):
    for sp in SPECIALS:
        width = len(sp.encode())
        for off in range(length - width + 1):
            ids = []
            for base in "abc":
                clean = base * length
                ids += [clean, clean[:off] + sp + clean[off + 1:][:length - off - width]]
            assert {len(i.encode()) for i in ids} == {length}
            ids.sort()
            check(ids)        # the run
            check(ids[::-1])  # the fallback


def test_every_entry_needs_escaping():
    check(['"' * 8] * 300)
    check(["\x01" * 16] * 300)
    check(["\x02" * 5] * 300 + ["\x01" * 5])


# ---- truncation -------------------------------------------------------------

@pytest.mark.parametrize("length", [1, 2, 5, 7, 8, 9, 16])
def test_every_truncation_raises_or_is_a_shorter_message(length):
    """a cut inside an entry must raise; a cut on an entry boundary gives the
    digest of the IDs before it (the criterion of digest_selftest.cpp)"""
    sorted_ids = sorted(fixed_ids(6, length, random.Random(length)))
    for ids in (sorted_ids, sorted_ids[::-1]):
        msg = id_list(ids)
        for k in range(len(msg) + 1):
            cut = bytes(msg[:k])
            if k % (length + 2) == 0:
                check_body(ids[:k // (length + 2)], cut)
            else:
                for fn, arg in ((_fastwire.decode_prestart_digest, cut),
                                (_fastwire.decode_prestart_digest2, cut),
                                (_fastwire.digest_allocate_request, ld(1, cut))):
                    with pytest.raises(RuntimeError):
                        fn(arg)


# ---- shuffled input ---------------------------------------------------------

@pytest.mark.parametrize("length", range(1, 10))
def test_shuffled_fixed_width_sets(length):
    rng = random.Random(100 + length)
    for n in (2, 255, 256, 257):
        ids = fixed_ids(n, length, rng)
        check(ids)
        assert (_fastwire.decode_prestart_digest2(id_list(ids))
                == _fastwire.decode_prestart_digest2(id_list(sorted(ids))))
        check(fixed_ids(n, length, rng, alphabet="01"))          # duplicates
        check(fixed_ids(n, length, rng, alphabet="\x00\x7f"))    # key byte 0x00


def test_shuffled_18432():
    ids = [f"1-{i:06d}" for i in range(18432)]
    shuffled = list(ids)
    random.Random(5).shuffle(shuffled)
    want = ref(ids)
    body, body_sorted = id_list(shuffled), id_list(ids)
    for b in (body, body_sorted):
        assert _fastwire.decode_prestart_digest2(b) == (want[0], want[1], want[3])
        assert _fastwire.digest_allocate_request(ld(1, b)) == [want[:2]]
        assert _fastwire.decode_prestart_digest(b) == (want[2], want[0])


def test_shuffled_key_bytes_00_and_ff():
    """raw 0xFF bytes are not UTF-8, so only the entry points that return no
    strings take them; the hash and the order are defined on bytes"""
    import hashlib
    rng = random.Random(9)
    for length in range(1, 10):
        for n in (2, 255, 256, 257):
            raw = [bytes(rng.choice(b"\x00\xff\x30") for _ in range(length)) for _ in range(n)]
            body = b"".join(ld(1, r) for r in raw)
            h = hashlib.sha256(b":".join(sorted(raw))).hexdigest()[:8]
            assert _fastwire.digest_allocate_request(ld(1, body)) == [(h, n)]
            rows = _fastwire.podresources_digest(
                podresources_one(b"".join(ld(2, r) for r in raw)))
            assert rows == [("ns", "pod", "c", "res", h, n)]


def test_shuffled_mixed_lengths():
    rng = random.Random(11)
    ids = fixed_ids(300, 4, rng) + fixed_ids(300, 5, rng) + [""]
    rng.shuffle(ids)
    check(ids)
    check(fixed_ids(300, 6, rng) + ["0-00000"])  # one shorter ID at the very end


# ---- scratch reuse ----------------------------------------------------------

def test_large_request_then_small_one():
    """300,000 IDs take the scratch above its retention cap, so it is
    released on exit and regrown by the next call"""
    big = [f"0-{i:06d}" for i in range(300_000)]
    joined = ":".join(big)
    import hashlib
    h = hashlib.sha256(joined.encode()).hexdigest()[:8]
    body = id_list(big)
    small = ["0-3", "0-1", "0-2"]
    h2, n2, frag2 = _fastwire.decode_prestart_digest2(body)
    assert (h2, n2) == (h, 300_000)
    assert frag2 == ('["' + joined.replace(":", '","') + '"]').encode()
    check(small)
    # the same set unsorted: the key vector above the cap too
    rot = id_list(big[1:] + big[:1])
    assert _fastwire.decode_prestart_digest2(rot) == (h2, n2, frag2)
    check(small)
    assert _fastwire.digest_allocate_request(ld(1, rot)) == [(h, 300_000)]
    check(sorted(small))


def test_two_threads_keep_their_own_scratch():
    sets = {}
    for gpu in "34":
        ids = [f"{gpu}-{i:05d}" for i in range(3000)]
        shuffled = ids[1500:] + ids[:1500]
        sets[gpu] = (id_list(ids), id_list(shuffled), ref(ids))
    errors = []
    barrier = threading.Barrier(2)

    def worker(gpu):
        body, shuffled, want = sets[gpu]
        try:
            barrier.wait(timeout=30)
            for _ in range(40):
                for b in (body, shuffled):
                    assert _fastwire.decode_prestart_digest2(b) == (want[0], want[1], want[3])
                    assert _fastwire.digest_allocate_request(ld(1, b)) == [want[:2]]
                assert _fastwire.decode_prestart_digest(shuffled) == (want[2], want[0])
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(g,)) for g in sets]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
