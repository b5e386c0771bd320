"""Replay the fuzz corpus through the Python-visible parser entry points.

The libFuzzer harness (native/fuzz_targets.cpp, built by
`python -m elastic_gpu_agent_amd.native.build_fuzz`) drives the same code
with ASan; this replay keeps every interesting/crashing input from past
fuzzing sessions in the normal CPU suite. First catch: a 64-bit
length-varint pointer-wrap OOB read in the wire walker
(wirecore.h Reader/spans_of — fixed; the crash input is in the corpus).
"""
import glob
import os

import pytest

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_regressions_corpus")


def _inputs():
    return sorted(glob.glob(os.path.join(CORPUS, "*")))


@pytest.mark.skipif(not _inputs(), reason="no fuzz corpus checked in")
def test_replay_corpus_through_parsers():
    from elastic_gpu_agent_amd import _fastwire
    from elastic_gpu_agent_amd.protos import fastpath

    n = 0
    for path in _inputs():
        with open(path, "rb") as f:
            raw = f.read()
        if not raw:
            continue
        data = raw[1:]  # fuzz harness selector byte
        # every parser must either parse or raise cleanly — never crash
        for fn in (
            _fastwire.decode_string_list,
            _fastwire.decode_nested_string_lists,
            _fastwire.digest_allocate_request,
            _fastwire.decode_prestart_digest2,
            _fastwire.podresources_digest,
            fastpath.decode_preferred_request_digest,
        ):
            try:
                fn(data)
            except Exception:
                pass
        n += 1
    assert n >= 1


def test_wire_pointer_wrap_regression():
    """Direct regression for the fuzz-found OOB: a LEN field whose varint
    length wraps 64-bit pointer arithmetic must raise, not read wild."""
    from elastic_gpu_agent_amd import _fastwire

    # field 1, wire type 2, length = a huge 10-byte varint
    evil = bytes([0x0A]) + b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01"
    # also: huge length on a SKIPPED (non-1) field reaches Reader::skip
    evil_skip = bytes([0x12]) + b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01"
    for data in (evil, evil_skip, evil + b"AA", evil_skip + b"AA"):
        for fn in (
            _fastwire.decode_string_list,
            _fastwire.digest_allocate_request,
            _fastwire.decode_prestart_digest2,
            _fastwire.podresources_digest,
        ):
            with pytest.raises(Exception):
                fn(data)
