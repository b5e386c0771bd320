"""Where a large Allocate request's time goes: digest alone vs. the full RPC,
with the process's minor page faults, system time and voluntary context
switches per call (getrusage) next to the wall times. The sha256 row (hashlib
over the joined IDs) is the floor of the digest rows; the shuffled rows are
what kubelet's unsorted lists cost. decode_prestart_digest3 is what PreStart
calls (a large consecutive set comes back as ID runs); expand_runs is what a
reader of the stored record pays to get the list back. The hash-memo rows set
PreStart's digest after an Allocate of the same set (a hit: no second sha256)
against the same call with the memo off, and Allocate's digest with the memo
on (it also splits the set into runs and stores the fragment) against off; the
last two rows are a bind's file effects (two symlinks and the limits file)
through the Python calls and through the native ones.

  python tools/decompose_alloc.py              # 18,432 IDs: the mixed config
  python tools/decompose_alloc.py --ids 73728  # a 72-GiB pod at 1-MiB units
  python tools/decompose_alloc.py --id-format "0-{:011d}"  # 13-byte IDs: the
                                               # digest's two-word keys

Run from the repository root.
"""
import argparse, hashlib, json, os, random, resource, sys, time, tempfile
REPO = os.getcwd()
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from elastic_gpu_agent_amd import consts, egrpc, _fastwire
from elastic_gpu_agent_amd.isolation import LimitsWriter
from elastic_gpu_agent_amd.operator import GPUOperator
from elastic_gpu_agent_amd.protos import fastpath, deviceplugin as dp
from helpers import Harness

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--ids", type=int, default=18432,
                help="device IDs in the large request (default: 18432)")
ap.add_argument("--calls", type=int, default=300, help="timed calls per row")
ap.add_argument("--no-preferred", action="store_true",
                help="skip the 295k-pool GetPreferredAllocation row")
ap.add_argument("--id-format", default="0-{:06d}",
                help="str.format pattern of a device ID (default: 0-{:06d})")
args = ap.parse_args()

tmp = tempfile.mkdtemp(); h = Harness(tmp, gpus=1, mem_unit_mib=1)
h.plugin.memory_server.serve(); h.plugin.memory_server.wait_ready()
ch = egrpc.Channel(h.plugin.memory_server.socket_path)
raw = ch.unary_unary(dp.METHOD_ALLOCATE)
ids = [args.id_format.format(i) for i in range(args.ids)]
enc = fastpath.encode_allocate_request({"container_requests":[{"devicesIDs": ids}]})
shuffled = list(ids); random.Random(0).shuffle(shuffled)
enc_shuf = fastpath.encode_allocate_request({"container_requests":[{"devicesIDs": shuffled}]})
pre_enc = _fastwire.encode_string_list(ids)
pre_enc_shuf = _fastwire.encode_string_list(shuffled)
joined = ":".join(ids).encode()  # what the digest hashes: the floor of both digest rows
print(f"{'':42s} {'us':>8s} {'minflt':>8s} {'sys us':>8s} {'user us':>8s} {'vcsw':>6s}   (per call)")
def t(label, fn, n=args.calls, before=None):
    # `before` runs ahead of every call and is left out of the wall time (the
    # rusage columns include it)
    for _ in range(2):
        if before: before()
        fn()
    r0 = resource.getrusage(resource.RUSAGE_SELF)
    dt = 0.0
    for _ in range(n):
        if before: before()
        t0=time.perf_counter()
        fn()
        dt += time.perf_counter()-t0
    r1 = resource.getrusage(resource.RUSAGE_SELF)
    print(f"{label:42s} {dt/n*1e6:8.0f} {(r1.ru_minflt-r0.ru_minflt)/n:8.1f} "
          f"{(r1.ru_stime-r0.ru_stime)/n*1e6:8.0f} {(r1.ru_utime-r0.ru_utime)/n*1e6:8.0f} "
          f"{(r1.ru_nvcsw-r0.ru_nvcsw)/n:6.1f}")
print("ids:", args.ids, " req bytes:", len(enc))
t("sha256 of the joined bytes alone", lambda: hashlib.sha256(joined).hexdigest())
t("digest_allocate_request (C++ alone)", lambda: _fastwire.digest_allocate_request(enc))
t("digest_allocate_request, shuffled IDs", lambda: _fastwire.digest_allocate_request(enc_shuf))
t("decode_prestart_digest2 (C++ alone)", lambda: _fastwire.decode_prestart_digest2(pre_enc))
t("decode_prestart_digest2, shuffled IDs", lambda: _fastwire.decode_prestart_digest2(pre_enc_shuf))
t("decode_prestart_digest3 (C++ alone)", lambda: _fastwire.decode_prestart_digest3(pre_enc))
t("decode_prestart_digest3, shuffled IDs", lambda: _fastwire.decode_prestart_digest3(pre_enc_shuf))
_, _n, _frag, _is_runs = _fastwire.decode_prestart_digest3(pre_enc)
if _is_runs:  # what a reader of the stored record pays to get the list back
    t("expand_runs (runs -> list fragment)", lambda: _fastwire.expand_runs(_frag, _n))
# hash memo: PreStart after an Allocate of the same set takes Allocate's hash
memo_cap = _fastwire.hash_memo_stats()["cap"]
t("decode_prestart_digest3 after Allocate (hit)",
  lambda: _fastwire.decode_prestart_digest3(pre_enc),
  before=lambda: _fastwire.digest_allocate_request(enc))
t("digest_allocate_request, memo on", lambda: _fastwire.digest_allocate_request(enc))
_fastwire.hash_memo_configure(0)
t("decode_prestart_digest3, memo off",
  lambda: _fastwire.decode_prestart_digest3(pre_enc),
  before=lambda: _fastwire.digest_allocate_request(enc))
t("digest_allocate_request, memo off", lambda: _fastwire.digest_allocate_request(enc))
_fastwire.hash_memo_configure(memo_cap)
# a bind's file effects: two symlinks and the limits file
fx = tempfile.mkdtemp()
fx_pairs = [("/dev/dri/renderD128", os.path.join(fx, "elastic-gpu-feed0001-0")),
            ("/dev/kfd", os.path.join(fx, "elastic-gpuctl-feed0001-0"))]
fx_rec = {"version": 1, "gpu_indexes": [0], "render_minors": [128],
          "uuids": ["GPU-00000000000000000000000000000000"],
          "mem_limit_bytes": args.ids << 20}
fx_limits = os.path.join(fx, "feed0001.json")
def fx_clear():
    for _, link in fx_pairs:
        if os.path.lexists(link): os.unlink(link)
def fx_python():
    os.makedirs(fx, exist_ok=True)
    for target, link in fx_pairs: GPUOperator._force_symlink(target, link)
    fd, tmpname = tempfile.mkstemp(dir=fx, suffix=".tmp")
    with os.fdopen(fd, "w") as f: json.dump(fx_rec, f)
    os.replace(tmpname, fx_limits)
def fx_native():
    _fastwire.make_links(fx_pairs)
    _fastwire.atomic_write(fx_limits, json.dumps(fx_rec).encode())
t("links + limits file, Python path", fx_python, before=fx_clear)
t("links + limits file, native path", fx_native, before=fx_clear)
t("wire+server full (pre-encoded)", lambda: raw(enc))
small = fastpath.encode_allocate_request({"container_requests":[{"devicesIDs": ids[:20]}]})
t("wire+server (20 ids)", lambda: raw(small))
if not args.no_preferred:
    # GetPreferredAllocation at full 295k pool
    pool = [f"0-{i:06d}" for i in range(295_000)]
    pref_enc = dp.PreferredAllocationRequest.encode({"container_requests":[
        {"available_deviceIDs": pool, "allocation_size": 73728}]})
    pref_raw = ch.unary_unary(dp.METHOD_GET_PREFERRED_ALLOCATION)
    print("pref req bytes:", len(pref_enc))
    t("GetPreferred wire+server (295k pool)", lambda: pref_raw(pref_enc), n=15)
ch.close(); h.close()
