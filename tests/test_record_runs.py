"""Large device sets stored as ID runs: the native codec against a plain
definition written here, its rejections, the store round trip through both
record formats, and the pure-Python fallback.

The reference list fragment is json.dumps(sorted_ids, separators=(",", ":"))
throughout; no timing is asserted anywhere in this file.
"""
import json
import random
import sqlite3

import pytest

from elastic_gpu_agent_amd import consts
from elastic_gpu_agent_amd.protos import fastpath
from elastic_gpu_agent_amd.types import Device, PodContainer, PodInfo

_fastwire = pytest.importorskip("elastic_gpu_agent_amd._fastwire")

MIN_IDS, PER = 1024, 8


# ---- the format, spelled out independently of fastpath.py -------------------

def ref_split(s):
    i = len(s)
    while i > 0 and s[i - 1] in "0123456789":
        i -= 1
    width = len(s) - i
    if not 1 <= width <= 18:
        return None
    if any(ord(c) < 0x20 or ord(c) >= 0x80 or c in '"\\' for c in s):
        return None
    return s[:i], width, int(s[i:])


def ref_runs(sorted_ids):
    """The runs of a sorted set, or None where it keeps its literal list."""
    runs = []
    prev = None
    for s in sorted_ids:
        t = ref_split(s)
        if t is None:
            return None
        if prev is not None and t[:2] == prev[:2] and t[2] == prev[2] + 1:
            runs[-1][3] += 1
        else:
            runs.append([t[0], t[1], t[2], 1])
        prev = t
    if len(sorted_ids) < MIN_IDS or len(runs) > len(sorted_ids) // PER:
        return None
    return runs


def list_fragment(sorted_ids):
    # the digest copies bytes >= 0x80 through, as its own tests pin
    return json.dumps(sorted_ids, separators=(",", ":"), ensure_ascii=False).encode()


def mem_ids(n, gpu=0, start=0):
    return [f"{gpu}-{i:06d}" for i in range(start, start + n)]


def fragmented(nruns, per=8):
    return [i for r in range(nruns) for i in mem_ids(per, start=r * 100)]


CASES = {
    "1023": mem_ids(1023),
    "1024": mem_ids(1024),
    "1025": mem_ids(1025),
    "runs-at-count/8": fragmented(128),          # 1024 IDs, 128 runs
    "runs-at-count/8+1": fragmented(128)[:-1],   # 1023 IDs: below the minimum too
    "runs-over-count/8": fragmented(129) + mem_ids(6, start=90000),  # 1038 IDs, 130 runs
    "one-run": mem_ids(18432),
    "two-gpus": mem_ids(700, 0) + mem_ids(700, 1),
    "gap": [i for i in mem_ids(2000) if i != "0-000777"],
    "duplicate": sorted(mem_ids(2000) + ["0-000005"]),
    "rollover-in-width": mem_ids(2000, start=99000),   # 0-099999, 0-100000
    "width-change": sorted([f"7-{i}" for i in range(1, 1200)]),  # sorted, it is fragments
    "18-digits": [f"a{i:018d}" for i in range(1500)],
    "19-digits": [f"a{i:019d}" for i in range(1500)],
    "top-of-width": [f"a{i:04d}" for i in range(8000, 10000)],
    "no-digits": sorted(mem_ids(2000) + ["0-abc"]),
    "needs-escape": sorted(mem_ids(2000) + ['0-"1']),
    "control-byte": sorted(mem_ids(2000) + ["0-\x01" + "1"]),
    "non-ascii": sorted(mem_ids(2000) + ["é1"]),
    "colon-in-prefix": [f"a:b:{i:05d}" for i in range(1500)],
    "mixed-lengths": sorted(mem_ids(1500) + [f"10-{i:06d}" for i in range(1500)]
                            + [f"gpu-long-prefix-{i:08d}" for i in range(1500)]),
    "long-ids": [f"gpu-long-prefix-{i:08d}" for i in range(1500)],   # above the stride cap
    "nine-byte-ids": [f"10-{i:06d}" for i in range(1500)],           # two-word stride path
    "short-ids": [f"{i:03d}" for i in range(1000)] + [f"a{i:02d}" for i in range(100)],
}
# what each case must come out as, by the definition above
for _name in ("1024", "1025", "runs-at-count/8", "one-run", "two-gpus", "gap", "duplicate",
              "rollover-in-width", "18-digits", "top-of-width",
              "colon-in-prefix", "mixed-lengths", "long-ids", "nine-byte-ids", "short-ids"):
    assert ref_runs(sorted(CASES[_name])) is not None, _name
for _name in ("1023", "runs-at-count/8+1", "runs-over-count/8", "width-change", "19-digits",
              "no-digits", "needs-escape", "control-byte", "non-ascii"):
    assert ref_runs(sorted(CASES[_name])) is None, _name


@pytest.mark.parametrize("name", sorted(CASES))
def test_codec_matches_definition(name):
    ids = sorted(CASES[name])
    runs = ref_runs(ids)
    want_runs = None if runs is None else json.dumps(runs, separators=(",", ":")).encode()
    frag = list_fragment(ids)
    d = Device.new(ids)

    assert _fastwire.ids_to_runs(ids) == want_runs
    shuffled = list(ids)
    random.Random(7).shuffle(shuffled)
    for order in (ids, shuffled):
        body = _fastwire.encode_string_list(order)
        h, n, got, is_runs = _fastwire.decode_prestart_digest3(body)
        assert (h, n) == (d.hash, len(ids))
        # digest2 stays what it was
        assert _fastwire.decode_prestart_digest2(body) == (d.hash, len(ids), frag)
        if want_runs is None:
            assert (got, is_runs) == (frag, False)
        else:
            assert (got, is_runs) == (want_runs, True)
            assert len(got) < len(frag)
    if want_runs is not None:
        assert _fastwire.expand_runs(want_runs, len(ids)) == frag


def test_width_change_starts_a_run():
    """...9 then ...10: byte order never puts the two side by side under one
    prefix, so this goes to the codec in numeric order, which it keeps."""
    ids = [f"a{i}" for i in range(1, 2000)]
    runs = _fastwire.ids_to_runs(ids)
    assert json.loads(runs) == [["a", 1, 1, 9], ["a", 2, 10, 90], ["a", 3, 100, 900],
                                ["a", 4, 1000, 1000]]
    assert fastpath._py_ids_to_runs(ids) == runs
    assert _fastwire.expand_runs(runs, len(ids)) == list_fragment(ids)
    assert fastpath._py_expand_runs(runs, len(ids)) == list_fragment(ids)


def test_shuffled_mixed_lengths_take_the_span_sort():
    """IDs of several lengths, unsorted: the fallback that sorts spans (not
    the radix sort) must hand the same runs to the builder."""
    ids = CASES["mixed-lengths"]
    shuffled = list(ids)
    random.Random(3).shuffle(shuffled)
    a = _fastwire.decode_prestart_digest3(_fastwire.encode_string_list(sorted(ids)))
    b = _fastwire.decode_prestart_digest3(_fastwire.encode_string_list(shuffled))
    assert a == b and a[3] is True
    assert json.loads(a[2]) == [["0-", 6, 0, 1500], ["10-", 6, 0, 1500],
                                ["gpu-long-prefix-", 8, 0, 1500]]


def test_fastpath_returns_runs_or_todays_dict():
    big, small = mem_ids(2048), [f"0-{i:02d}" for i in range(30)]
    req = fastpath.decode_prestart_request_digest(fastpath.encode_prestart_request({"devicesIDs": big}))
    assert req == {"devicesIDs": [], "device_hash": Device.new(big).hash, "device_count": 2048,
                   "list_runs": b'[["0-",6,0,2048]]'}
    req = fastpath.decode_prestart_request_digest(fastpath.encode_prestart_request({"devicesIDs": small}))
    assert req == {"devicesIDs": [], "device_hash": Device.new(small).hash, "device_count": 30,
                   "list_json": list_fragment(small)}


@pytest.mark.parametrize("frag,count", [
    (b'[["0-",6,0,2048]]', 2047),            # wrong N, either way
    (b'[["0-",6,0,2048]]', 2049),
    (b'[["0-",6,0,1000],["0-",6,2000,1000]]', 1000),
    (b'[["0-",6,999000,1001]]', 1001),       # start + count past 10^width
    (b'[["0-",1,9,2]]', 2),
    (b'[["0-",0,0,1]]', 1),                  # width 0 and 19
    (b'[["0-",19,0,1]]', 1),
    (b'[["0-",6,-1,5]]', 5),                 # negative, non-integer, wrong type
    (b'[["0-",6,0,-5]]', 5),
    (b'[["0-",6,0.0,5]]', 5),
    (b'[["0-",6,0,5e0]]', 5),
    (b'[["0-",6,"0",5]]', 5),
    (b'[["0-",6,0,true]]', 1),
    (b'[[0,6,0,5]]', 5),
    (b'[["0-",6,0,0]]', 0),                  # an empty run
    (b'[["0-",6,0,5,1]]', 5),
    (b'[["0-",6,0]]', 0),
    (b'[["0-",6,0,2048]', 2048),             # truncated JSON, at every level
    (b'[["0-",6,0,20', 20),
    (b'[["0-', 0),
    (b'[', 0),
    (b'', 0),
    (b'[["0-",6,0,5]]x', 5),
    (b'[["0\\u002d",6,0,5]]', 5),            # prefixes are never escaped
    (b'[["0-",18,0,600000]]', 600000),       # 600000 * 23 bytes: over the 4 MiB cap
    (b'[["0-",6,0,99999999999999999999]]', 5),
    (b'{"0-":[6,0,5]}', 5),
])
def test_expand_runs_rejects(frag, count):
    for expand in (_fastwire.expand_runs, fastpath._py_expand_runs):
        with pytest.raises(Exception) as ei:
            expand(frag, count)
        assert not isinstance(ei.value, (MemoryError, SystemError)), ei.value


def test_expand_runs_accepts_what_the_encoder_never_writes():
    assert _fastwire.expand_runs(b"[]", 0) == b"[]"
    assert _fastwire.expand_runs(b' [ [ "0-" , 2 , 98 , 2 ] ] ', 2) == b'["0-98","0-99"]'
    assert fastpath._py_expand_runs(b' [ [ "0-" , 2 , 98 , 2 ] ] ', 2) == b'["0-98","0-99"]'
    with pytest.raises(Exception):
        _fastwire.expand_runs(b'[["0-",6,0,5]]', -1)


def test_fuzz_seeds_through_the_python_entry_points():
    """The checked-in seeds of the fuzz harness (tests/golden/fuzz_runs_seeds:
    a selector byte, then a wire body or a 16-bit count and a runs fragment)
    parse or raise cleanly, and where a wire body comes back as runs they
    expand to what digest2 gives."""
    import glob
    import os

    seeds = sorted(glob.glob(os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_runs_seeds", "*")))
    assert len(seeds) == 8
    for path in seeds:
        with open(path, "rb") as f:
            raw = f.read()
        if raw[0] == 3:  # AllocateRequest shape: one container
            assert raw[1] == 0x0A  # field 1, then the body's length varint
            end_of_len = next(i for i in range(2, len(raw)) if raw[i] < 0x80)
            inner = raw[end_of_len + 1:]
            h, n, frag, is_runs = _fastwire.decode_prestart_digest3(inner)
            h2, n2, frag2 = _fastwire.decode_prestart_digest2(inner)
            assert (h, n) == (h2, n2)
            assert (_fastwire.expand_runs(frag, n) if is_runs else frag) == frag2
            assert is_runs == ("not-encodable" not in path)
        else:
            assert raw[0] == 4
            count = int.from_bytes(raw[1:3], "little")
            outcomes = []
            for expand in (_fastwire.expand_runs, fastpath._py_expand_runs):
                try:
                    outcomes.append(expand(raw[3:], count))
                except RuntimeError:
                    outcomes.append(None)
            assert outcomes[0] == outcomes[1]
            assert (outcomes[0] is not None) == path.endswith("runs-fragment-good")


# ---- types -------------------------------------------------------------------

def test_device_runs_form_stays_reference_format():
    ids = mem_ids(2048)
    d = Device.new(ids, consts.RESOURCE_GPU_MEMORY)
    r = Device.from_runs(d.hash, 2048, b'[["0-",6,0,2048]]', consts.RESOURCE_GPU_MEMORY)
    assert r.n_ids == 2048 and r.ids() == d.list
    assert r.equals(d) and d.equals(r)
    assert r.to_json_obj() == d.to_json_obj()
    assert r.to_json_bytes() == d.to_json_bytes()
    stored = r.to_stored_bytes()
    assert stored == d.to_stored_bytes()  # Device.new compresses through ids_to_runs
    assert json.loads(stored) == {"Hash": d.hash, "Runs": [["0-", 6, 0, 2048]], "N": 2048,
                                  "ResourceName": consts.RESOURCE_GPU_MEMORY}
    small = Device.new(ids[:30], consts.RESOURCE_GPU_CORE)
    assert small.to_stored_bytes() == small.to_json_bytes()
    lazy = Device.from_digest(small.hash, 30, list_fragment(ids[:30]), consts.RESOURCE_GPU_CORE)
    assert lazy.to_stored_bytes() == small.to_json_bytes()


def test_podinfo_from_raw_reads_both_shapes_and_checks_n():
    big = Device.new(mem_ids(2048), consts.RESOURCE_GPU_MEMORY)
    small = Device.new([f"0-{i:02d}" for i in range(30)], consts.RESOURCE_GPU_CORE)
    pi = PodInfo("ns", "p", {"m": big, "c": small})
    assert pi.val() == json.dumps(
        {"m": big.to_json_obj(), "c": small.to_json_obj()}, separators=(",", ":")).encode()
    stored = pi.stored_val()
    assert len(stored) < 1024 < len(pi.val())
    for raw in (stored, pi.val()):
        back = PodInfo.from_raw("ns/p", raw)
        assert back.val() == pi.val()
        assert back.stored_val() == stored
        assert back.container_device_map["m"].equals(big)
        assert back.container_device_map["m"].n_ids == 2048
    for bad in (b'{"m":{"Hash":"x","Runs":[["0-",6,0,2048]],"N":2047,"ResourceName":"r"}}',
                b'{"m":{"Hash":"x","Runs":[["0-",6,0,2048]],"ResourceName":"r"}}',
                b'{"m":{"Hash":"x","Runs":[["0-",6,0]],"N":0,"ResourceName":"r"}}',
                b'{"m":{"Hash":"x","Runs":[["0-",6,0,-1]],"N":-1,"ResourceName":"r"}}'):
        with pytest.raises(ValueError):
            PodInfo.from_raw("ns/p", bad)
    # N agrees with the sum but a run overflows its width: caught on expansion
    odd = PodInfo.from_raw(
        "ns/p", b'{"m":{"Hash":"x","Runs":[["0-",1,5,10]],"N":10,"ResourceName":"r"}}')
    with pytest.raises(Exception):
        odd.container_device_map["m"].ids()


# ---- the store -----------------------------------------------------------------

BIG = mem_ids(2048)
SMALL = [f"0-{i:02d}" for i in range(30)]


def _prestart_both(plugin, sitter_add, core_locator, mem_locator):
    """PreStart of a 2,048-ID memory set (pod ns/mem) and a 30-ID core set
    (pod ns/core) through the wire decoder."""
    for name, ids, res, plug, loc in (
            ("mem", BIG, consts.RESOURCE_GPU_MEMORY, plugin.memory, mem_locator),
            ("core", SMALL, consts.RESOURCE_GPU_CORE, plugin.core, core_locator)):
        d = Device.new(ids, res)
        loc.assign(d.hash, PodContainer("ns", name, "main"))
        sitter_add("ns", name, "main", "0")
        req = fastpath.decode_prestart_request_digest(
            fastpath.encode_prestart_request({"devicesIDs": ids}))
        assert plug.pre_start_container(req, None) == {}


def _raw_vals(db_path):
    conn = sqlite3.connect(db_path)
    try:
        return {k: bytes(v) for k, v in conn.execute("SELECT key, val FROM pods")}
    finally:
        conn.close()


def _expected():
    return {
        "ns/mem": PodInfo("ns", "mem", {"main": Device.new(BIG, consts.RESOURCE_GPU_MEMORY)}),
        "ns/core": PodInfo("ns", "core", {"main": Device.new(SMALL, consts.RESOURCE_GPU_CORE)}),
    }


def test_store_round_trip_runs(tmp_path, capsys):
    from elastic_gpu_agent_amd.cli import egpuctl
    from elastic_gpu_agent_amd.storage.boltcompat import read_bolt_bucket
    from helpers import Harness

    h = Harness(str(tmp_path), gpus=1, mem_unit_mib=1)
    try:
        _prestart_both(h.plugin, h.add_assumed_pod, h.core_locator, h.mem_locator)
        want = _expected()
        raw = _raw_vals(h.storage.path)
        assert len(raw["ns/mem"]) < 1024
        assert json.loads(raw["ns/mem"]) == {"main": {
            "Hash": want["ns/mem"].container_device_map["main"].hash,
            "Runs": [["0-", 6, 0, 2048]], "N": 2048,
            "ResourceName": consts.RESOURCE_GPU_MEMORY}}
        assert raw["ns/core"] == want["ns/core"].val()

        for key, pi in want.items():
            got = h.storage.load("ns", pi.name).container_device_map["main"]
            ref = pi.container_device_map["main"]
            assert (got.ids(), got.n_ids, got.hash) == (ref.list, len(ref.list), ref.hash)
            assert got.equals(ref)
        seen = {}
        h.storage.for_each(lambda pi: seen.__setitem__(pi.key(), pi.val()))
        assert seen == {k: pi.val() for k, pi in want.items()}

        bolt = str(tmp_path / "export.bolt")
        assert egpuctl.main(["--db", h.storage.path, "export-bolt", "--to", bolt]) == 0
        assert dict(read_bolt_bucket(bolt, b"root")) == {
            k.encode(): pi.val() for k, pi in want.items()}
        capsys.readouterr()
        assert egpuctl.main(["--db", h.storage.path, "pods"]) == 0
        units = {r["pod"]: r["containers"]["main"]["units"]
                 for r in json.loads(capsys.readouterr().out)}
        assert units == {"ns/mem": 2048, "ns/core": 30}
    finally:
        h.close()


def test_store_record_format_list(tmp_path, monkeypatch):
    """--recordFormat list reaches the store and restores the parent's rows."""
    from elastic_gpu_agent_amd import manager as manager_mod
    from elastic_gpu_agent_amd.cli import agent
    from elastic_gpu_agent_amd.kube.locator import FakeDeviceLocator
    from elastic_gpu_agent_amd.kube.pods import Pod
    from elastic_gpu_agent_amd.kube.sitter import FakeSitter
    from elastic_gpu_agent_amd.manager import GPUManager, ManagerOptions
    from elastic_gpu_agent_amd.plugins.config import AgentPaths, PluginOptions

    seen = {}

    class StopHere(Exception):
        pass

    def fake_manager(opts):
        seen["opts"] = opts
        raise StopHere

    monkeypatch.setattr(manager_mod, "GPUManager", fake_manager)
    with pytest.raises(StopHere):
        agent.main(["--backend", "fake"])
    assert seen["opts"].record_format == "runs" == ManagerOptions().record_format
    with pytest.raises(StopHere):
        agent.main(["--backend", "fake", "--recordFormat", "list"])
    assert seen["opts"].record_format == "list"
    with pytest.raises(SystemExit):
        agent.main(["--backend", "fake", "--recordFormat", "bolt"])
    assert ManagerOptions.from_json(seen["opts"].to_json()).record_format == "list"

    (tmp_path / "dp").mkdir()
    paths = AgentPaths(
        dev_root=str(tmp_path / "dev"), plugin_dir=str(tmp_path / "dp"),
        kubelet_socket=str(tmp_path / "dp" / "kubelet.sock"),
        limits_dir=str(tmp_path / "limits"), limits_dir_host=None,
        state_dir=str(tmp_path), shim_host_path=None)
    opts = ManagerOptions(backend="fake", db_path=str(tmp_path / "meta.db"), paths=paths,
                          plugin_options=PluginOptions(mem_unit_mib=1), record_format="list")
    sitter, core_loc, mem_loc = FakeSitter(), FakeDeviceLocator(), FakeDeviceLocator()
    mgr = GPUManager(opts, sitter=sitter, locators=(core_loc, mem_loc))

    def add_pod(ns, name, container, gpu_indexes):
        sitter.add(Pod(namespace=ns, name=name, annotations={
            consts.ELASTIC_GPU_ASSUMED_ANNOTATION: "true",
            consts.ELASTIC_GPU_CONTAINER_ANNOTATION % container: gpu_indexes}))

    try:
        _prestart_both(mgr.plugin, add_pod, core_loc, mem_loc)
        assert _raw_vals(opts.db_path) == {k: pi.val() for k, pi in _expected().items()}
        got = mgr.storage.load("ns", "mem").container_device_map["main"]
        assert got.list == tuple(BIG)
    finally:
        mgr.plugin.stop()
        mgr.storage.close()


def test_opening_with_list_format_rewrites_runs_rows(tmp_path):
    from elastic_gpu_agent_amd.storage import Storage, new_storage

    db = str(tmp_path / "db")
    want = _expected()
    st = Storage(db)
    for pi in want.values():
        st.save(pi)
    st.close()
    assert len(_raw_vals(db)["ns/mem"]) < 1024
    new_storage(db).close()  # the default leaves the rows alone
    assert len(_raw_vals(db)["ns/mem"]) < 1024
    st = new_storage(db, "list")
    try:
        assert _raw_vals(db) == {k: pi.val() for k, pi in want.items()}
        assert st.rewrite_as_lists() == 0
    finally:
        st.close()


def test_storage_rejects_unknown_record_format(tmp_path):
    from elastic_gpu_agent_amd.storage import Storage

    with pytest.raises(ValueError):
        Storage(str(tmp_path / "db"), record_format="bolt")


# ---- without the native module ---------------------------------------------------

def test_fallback_parity(monkeypatch):
    native = {}
    for name in sorted(CASES):
        ids = sorted(CASES[name])
        runs = fastpath.ids_to_runs(ids)
        native[name] = (runs, None if runs is None else fastpath.expand_runs(runs, len(ids)),
                        Device.new(ids, "r").to_stored_bytes())
    big_req = fastpath.encode_prestart_request({"devicesIDs": BIG})

    monkeypatch.setattr(fastpath, "_fastwire", None)
    for name in sorted(CASES):
        ids = sorted(CASES[name])
        runs = fastpath.ids_to_runs(ids)
        assert runs == native[name][0], name
        if runs is not None:
            assert fastpath.expand_runs(runs, len(ids)) == native[name][1] == list_fragment(ids), name
        assert Device.new(ids, "r").to_stored_bytes() == native[name][2], name
    # the wire decoder then hands over plain IDs, and the record is the same
    req = fastpath.decode_prestart_request_digest(big_req)
    assert "list_runs" not in req and req["devicesIDs"] == BIG
    d = Device.new(req["devicesIDs"], consts.RESOURCE_GPU_MEMORY)
    assert d.to_stored_bytes() == Device.from_runs(
        d.hash, 2048, b'[["0-",6,0,2048]]', consts.RESOURCE_GPU_MEMORY).to_stored_bytes()
