"""Build + (optionally) run the libFuzzer harness over the native parsers,
and the stand-alone sanitizer self-tests of the device-set digest, of the
ID-run codec the store uses, of the GPU self-test's host reference, of the
transport's HTTP/2 framing core, of the Allocate -> PreStart hash memo and of
the native file effects of a bind.

Usage:
  python -m elastic_gpu_agent_amd.native.build_fuzz             # build only
  python -m elastic_gpu_agent_amd.native.build_fuzz --run 60    # fuzz 60 s
  python -m elastic_gpu_agent_amd.native.build_fuzz --replay    # in-tree corpus, once
  python -m elastic_gpu_agent_amd.native.build_fuzz --selftest  # ASan+UBSan digest cases
                                                                # (general, then fixed-stride/radix),
                                                                # then the ID-run codec,
                                                                # then selftest_ref.h,
                                                                # then h2frame.h,
                                                                # then the hash memo,
                                                                # then bindfx.h
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CLANGXX = os.environ.get(
    "EGPU_FUZZ_CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")


def build(out=None):
    out = out or os.path.join(REPO, "bin", "egpu-fuzz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [
        CLANGXX, "-O1", "-g", "-std=c++17",
        "-fsanitize=fuzzer,address",
        os.path.join(HERE, "fuzz_targets.cpp"),
        os.path.join(HERE, "devfilter.cpp"),
        "-I", HERE, "-o", out,
    ]
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


# checked-in inputs: findings of past sessions, and the seeds of the ID-run
# codec (wire bodies for the digest differential, stored runs fragments)
SEED_DIRS = [
    os.path.join(REPO, "tests", "fuzz_regressions_corpus"),
    os.path.join(REPO, "tests", "golden", "fuzz_runs_seeds"),
]


def run(binary, seconds=30, corpus=None):
    corpus = corpus or os.path.join(REPO, "tests", "fuzz_corpus")
    os.makedirs(corpus, exist_ok=True)
    # libFuzzer writes new units to the first directory only; the checked-in
    # ones are read as seeds
    cmd = [binary, corpus, *[d for d in SEED_DIRS if os.path.isdir(d)],
           f"-max_total_time={seconds}", "-max_len=65536",
           "-print_final_stats=1"]
    print("+", " ".join(cmd), flush=True)
    return subprocess.call(cmd)


def replay(binary, corpus=None):
    """Run every input of the checked-in corpus through the harness once."""
    dirs = [corpus] if corpus else [d for d in SEED_DIRS if os.path.isdir(d)]
    inputs = sorted(os.path.join(d, f) for d in dirs for f in os.listdir(d))
    cmd = [binary, *inputs]
    print("+", binary, f"<{len(inputs)} corpus inputs>", flush=True)
    return subprocess.call(cmd)


def build_selftest(out=None, source="digest_selftest.cpp"):
    """digest_selftest.cpp: wirecore.h's fused digest against a naive
    reference, as an ordinary program with ASan + UBSan (no fuzzer runtime)."""
    out = out or os.path.join(REPO, "bin", "egpu-digest-selftest")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [
        CLANGXX, "-O1", "-g", "-std=c++17", "-pthread",
        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
        os.path.join(HERE, source),
        "-I", HERE, "-o", out,
    ]
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build_stride_selftest(out=None):
    """digest_stride_selftest.cpp: the fixed-stride run and the radix
    fallback of the same digest, built the same way."""
    out = out or os.path.join(REPO, "bin", "egpu-digest-stride-selftest")
    return build_selftest(out, "digest_stride_selftest.cpp")


def build_runs_selftest(out=None):
    """runs_selftest.cpp: the ID-run codec of idruns.h (RunBuilder,
    expand_runs) under wirecore.h's digest_field_runs, built the same way."""
    out = out or os.path.join(REPO, "bin", "egpu-runs-selftest")
    return build_selftest(out, "runs_selftest.cpp")


def build_ref_selftest(out=None):
    """selftest_ref_selftest.cpp: the host reference of the GPU self-test
    (selftest_ref.h, no GPU code), built the same way."""
    out = out or os.path.join(REPO, "bin", "egpu-selftest-ref-selftest")
    return build_selftest(out, "selftest_ref_selftest.cpp")


def build_mx_ref_selftest(out=None):
    """selftest_mx_ref_selftest.cpp: the host reference of the matrix sweep
    (selftest_mx_ref.h: decoders, generator, expected signatures; no GPU
    code), built the same way."""
    out = out or os.path.join(REPO, "bin", "egpu-selftest-mx-ref-selftest")
    return build_selftest(out, "selftest_mx_ref_selftest.cpp")


def build_h2frame_selftest(out=None):
    """h2frame_selftest.cpp: the transport's receive buffer, frame parser and
    header-block builders (h2frame.h, no Python) over a socketpair, built the
    same way."""
    out = out or os.path.join(REPO, "bin", "egpu-h2frame-selftest")
    return build_selftest(out, "h2frame_selftest.cpp")


def build_hash_memo_selftest(out=None):
    """hash_memo_selftest.cpp: hashmemo.h's HashMemo and wirecore.h's two
    digests that share it, threaded case included, built the same way."""
    out = out or os.path.join(REPO, "bin", "egpu-hash-memo-selftest")
    return build_selftest(out, "hash_memo_selftest.cpp")


def build_bindfx_selftest(out=None):
    """bindfx_selftest.cpp: the symlink / temp-file-and-rename / unlink calls
    of bindfx.h in a scratch directory, threaded case included, built the
    same way."""
    out = out or os.path.join(REPO, "bin", "egpu-bindfx-selftest")
    return build_selftest(out, "bindfx_selftest.cpp")


if __name__ == "__main__":
    if "--selftest" in sys.argv:
        rc = subprocess.call([build_selftest()])
        rc = rc or subprocess.call([build_stride_selftest()])
        rc = rc or subprocess.call([build_runs_selftest()])
        rc = rc or subprocess.call([build_ref_selftest()])
        rc = rc or subprocess.call([build_mx_ref_selftest()])
        rc = rc or subprocess.call([build_h2frame_selftest()])
        rc = rc or subprocess.call([build_hash_memo_selftest()])
        sys.exit(rc or subprocess.call([build_bindfx_selftest()]))
    binary = build()
    if "--replay" in sys.argv:
        sys.exit(replay(binary))
    if "--run" in sys.argv:
        secs = int(sys.argv[sys.argv.index("--run") + 1])
        sys.exit(run(binary, secs))
