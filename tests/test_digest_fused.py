"""The four device-set digests of _fastwire (digest_allocate_request,
decode_prestart_digest, decode_prestart_digest2, podresources_digest) share
one fused walk -> order check -> join -> hash helper with reused per-thread
scratch buffers. Every case is compared against the Python definitions:
types.hash_device_ids / Device.new and json.dumps."""
import json
import os
import random
import subprocess
import sys

import pytest

from elastic_gpu_agent_amd import _fastwire
from elastic_gpu_agent_amd.types import Device, hash_device_ids

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def id_list(ids, field=1, between=b"") -> bytes:
    """repeated string `field`, with `between` after every entry"""
    return b"".join(ld(field, i.encode()) + between for i in ids)


# unknown fields of every wire type the walker accepts: varint, fixed64,
# length-delimited, fixed32 — and a field 1 that is NOT length-delimited
UNKNOWN = (varint(2 << 3 | 0) + varint(300)
           + varint(7 << 3 | 1) + b"\x01\x02\x03\x04\x05\x06\x07\x08"
           + ld(9, b"0-zzz-not-an-id")
           + varint(4 << 3 | 5) + b"\xaa\xbb\xcc\xdd"
           + varint(1 << 3 | 0) + varint(5))


def ref(ids):
    """(hash, count, sorted list, JSON fragment) by the Python definitions"""
    d = Device.new(ids)
    assert d.hash == hash_device_ids(sorted(ids))
    return (d.hash, len(ids), list(d.list),
            json.dumps(list(d.list), separators=(",", ":")).encode())


def check_all_entry_points(ids, between=b""):
    h, n, sorted_ids, frag = ref(ids)
    body = id_list(ids, between=between)
    # Allocate: one container request
    assert _fastwire.digest_allocate_request(ld(1, body)) == [(h, n)]
    # PreStart v1: sorted strings + hash
    got_list, got_hash = _fastwire.decode_prestart_digest(body)
    assert (got_list, got_hash) == (sorted_ids, h)
    # PreStart v2: hash, count, JSON fragment
    h2, n2, frag2 = _fastwire.decode_prestart_digest2(body)
    assert (h2, n2) == (h, n)
    assert frag2 == frag
    assert json.loads(frag2) == sorted_ids
    # podresources: the IDs are field 2 of ContainerDevices
    rows = _fastwire.podresources_digest(podresources([("ns", "pod", [("c", [("res", ids)])])],
                                                      between=between))
    assert rows == ([("ns", "pod", "c", "res", h, n)] if ids else [])


def podresources(pods, between=b"", one_entry_per_id=False) -> bytes:
    out = b""
    for ns, name, containers in pods:
        pod = ld(1, name.encode()) + ld(2, ns.encode())
        for cname, resources in containers:
            c = ld(1, cname.encode())
            for res, ids in resources:
                if one_entry_per_id:
                    for i in ids:
                        c += ld(2, ld(1, res.encode()) + ld(2, i.encode()))
                else:
                    c += ld(2, ld(1, res.encode()) + id_list(ids, field=2, between=between))
            pod += ld(3, c)
        out += ld(1, pod)
    return out


SORTED = [f"0-{i:04d}" for i in range(300)]
LAST_PAIR = SORTED[:-2] + [SORTED[-1], SORTED[-2]]

CASES = {
    "empty": [],
    "single": ["0-07"],
    "sorted": SORTED,
    "reverse": SORTED[::-1],
    "sorted_but_last_pair": LAST_PAIR,
    "duplicates_sorted": ["0-1", "0-1", "0-2", "0-2", "0-2"],
    "duplicates_unsorted": ["0-2", "0-1", "0-2", "0-1"],
    "prefix_neighbour": ["0-1", "0-10"],
    "prefix_neighbour_reversed": ["0-10", "0-1"],
    "zero_length_id": ["", "0-1"],
    "zero_length_id_last": ["0-1", ""],
    "only_zero_length": ["", ""],
    "len_127_128": ["a" * 127, "a" * 128],       # 1-byte -> 2-byte length varint
    "len_128_127": ["b" * 128, "a" * 127],
    "json_escapes": ['0-"q"', "0-\\b", "0-\x1f", '\x1f"\\'],
    "json_escapes_sorted": sorted(['0-"q"', "0-\\b", "0-\x1f", '\x1f"\\', "plain"]),
    "all_escapes_long": ['"' * 200, "\x1f" * 200],  # fragment 6x the input
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_entry_point_matches_python(name):
    check_all_entry_points(CASES[name])


@pytest.mark.parametrize("name", ["sorted", "reverse", "single", "json_escapes"])
def test_unknown_fields_between_ids(name):
    check_all_entry_points(CASES[name], between=UNKNOWN)


def test_shuffled_matches_sorted():
    ids = [f"{g}-{i:06d}" for g in range(3) for i in range(700)]
    shuffled = list(ids)
    random.Random(7).shuffle(shuffled)
    check_all_entry_points(shuffled)
    assert (_fastwire.decode_prestart_digest2(id_list(shuffled))
            == _fastwire.decode_prestart_digest2(id_list(ids)))


@pytest.mark.parametrize("n", [2, 3])
def test_several_container_requests(n):
    sets = [SORTED[:50], SORTED[50:10:-1], ["0-10", "", "0-1"]][:n]
    req = b"".join(ld(1, id_list(s)) + UNKNOWN for s in sets)
    assert _fastwire.digest_allocate_request(req) == [ref(s)[:2] for s in sets]


def test_podresources_groups_and_entry_per_id():
    """one ContainerDevices entry per resource (pre-1.21) and one per ID
    (after) describe the same sets; resources and containers stay apart"""
    a, b = SORTED[:40][::-1], ["1-5", "1-3", "1-4"]
    pods = [("ns1", "p1", [("c1", [("mem", a), ("core", b)]), ("c2", [("mem", b)])]),
            ("ns2", "p2", [("c1", [("mem", [])])])]
    want = [("ns1", "p1", "c1", "mem") + ref(a)[:2],
            ("ns1", "p1", "c1", "core") + ref(b)[:2],
            ("ns1", "p1", "c2", "mem") + ref(b)[:2]]
    assert _fastwire.podresources_digest(podresources(pods)) == want
    assert _fastwire.podresources_digest(podresources(pods, one_entry_per_id=True)) == want


def test_every_truncation_raises_or_is_a_shorter_message():
    """Cut a small valid message at every offset. A cut inside an entry must
    raise; a cut on an entry boundary is itself a valid message and must give
    the digest of the IDs before the cut — nothing after the cut may count.
    (Reads past the end are what the stand-alone sanitizer program is for.)"""
    ids = ["0-2", "", "0-1", "x" * 130, "0-3"]
    entries = [ld(1, i.encode()) for i in ids[:2]] + [UNKNOWN] + \
              [ld(1, i.encode()) for i in ids[2:]]
    msg = b"".join(entries)
    # offsets that end a whole field (each UNKNOWN sub-field included)
    boundaries = {0: []}
    off, seen = 0, []
    for e in entries:
        if e is UNKNOWN:
            sub = [varint(2 << 3 | 0) + varint(300),
                   varint(7 << 3 | 1) + b"\x01\x02\x03\x04\x05\x06\x07\x08",
                   ld(9, b"0-zzz-not-an-id"),
                   varint(4 << 3 | 5) + b"\xaa\xbb\xcc\xdd",
                   varint(1 << 3 | 0) + varint(5)]
            assert b"".join(sub) == UNKNOWN
            for s in sub:
                off += len(s)
                boundaries[off] = list(seen)
        else:
            off += len(e)
            seen.append(ids[len(seen)])
            boundaries[off] = list(seen)
    assert off == len(msg)
    for k in range(len(msg) + 1):
        cut = bytes(msg[:k])
        if k in boundaries:
            h, n, sorted_ids, frag = ref(boundaries[k])
            assert _fastwire.decode_prestart_digest(cut) == (sorted_ids, h), k
            assert _fastwire.decode_prestart_digest2(cut) == (h, n, frag), k
            assert _fastwire.digest_allocate_request(ld(1, cut)) == [(h, n)], k
        else:
            for fn, arg in ((_fastwire.decode_prestart_digest, cut),
                            (_fastwire.decode_prestart_digest2, cut),
                            (_fastwire.digest_allocate_request, ld(1, cut))):
                with pytest.raises(RuntimeError):
                    fn(arg)
    # the outer message truncated too: a container body longer than what is left
    whole = ld(1, msg)
    for k in range(1, len(whole)):
        with pytest.raises(RuntimeError):
            _fastwire.digest_allocate_request(bytes(whole[:k]))
    # and podresources, whose IDs sit three messages deep
    pr = podresources([("ns", "p", [("c", [("r", ids)])])])
    for k in range(1, len(pr)):
        with pytest.raises(RuntimeError):
            _fastwire.podresources_digest(bytes(pr[:k]))


def test_overlong_varint_raises():
    with pytest.raises(RuntimeError):
        _fastwire.decode_prestart_digest2(b"\x0a" + b"\xff" * 10 + b"\x01")
    with pytest.raises(RuntimeError):  # length far beyond the buffer
        _fastwire.decode_prestart_digest2(b"\x0a" + b"\xff" * 9 + b"\x01")


_SMALL = ["0-3", "0-1", "0-2"]
_FRESH = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from elastic_gpu_agent_amd import _fastwire
small = bytes.fromhex(sys.argv[2])
outer = bytes.fromhex(sys.argv[3])
l, h = _fastwire.decode_prestart_digest(small)
h2, n2, frag = _fastwire.decode_prestart_digest2(small)
print(json.dumps([_fastwire.digest_allocate_request(outer), [l, h], [h2, n2, frag.decode()]]))
"""


def test_no_scratch_state_leaks_between_calls():
    """A 20,000-ID call (sorted, then shuffled, then one that fails half-way)
    followed by a 3-ID call answers exactly as a fresh process does."""
    small = id_list(_SMALL)
    outer = ld(1, small)
    fresh = json.loads(subprocess.run(
        [sys.executable, "-c", _FRESH, REPO, small.hex(), outer.hex()],
        check=True, capture_output=True, text=True, timeout=60).stdout)
    h, n, sorted_ids, frag = ref(_SMALL)
    assert fresh == [[[h, n]], [sorted_ids, h], [h, n, frag.decode()]]

    def small_answers():
        l, hh = _fastwire.decode_prestart_digest(small)
        h2, n2, f2 = _fastwire.decode_prestart_digest2(small)
        return [[list(t) for t in _fastwire.digest_allocate_request(outer)],
                [l, hh], [h2, n2, f2.decode()]]

    big = [f"0-{i:06d}" for i in range(20000)]
    shuffled = list(big)
    random.Random(3).shuffle(shuffled)
    for ids in (big, shuffled):
        body = id_list(ids)
        want = ref(ids)
        assert _fastwire.decode_prestart_digest2(body) == (want[0], want[1], want[3])
        assert small_answers() == fresh
        assert _fastwire.digest_allocate_request(ld(1, body)) == [want[:2]]
        assert small_answers() == fresh
        assert _fastwire.decode_prestart_digest(body) == (want[2], want[0])
        assert small_answers() == fresh
    # a big call that throws after filling the scratch
    with pytest.raises(RuntimeError):
        _fastwire.decode_prestart_digest2(id_list(big) + b"\x0a\x7f")
    assert small_answers() == fresh
    # and the empty set after all that
    assert _fastwire.decode_prestart_digest2(b"") == ref([])[:2] + (b"[]",)
