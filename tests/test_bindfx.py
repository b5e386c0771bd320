"""The native file effects of a bind and of a GC pass (native/bindfx.h,
exported from _fastwire) against the Python implementations they replace:
GPUOperator._force_symlink, LimitsWriter._atomic_write's mkstemp / json.dump /
os.replace, and try: os.unlink."""
import errno
import io
import json
import os
import pathlib
import stat
import threading

import pytest

from elastic_gpu_agent_amd import consts
from elastic_gpu_agent_amd.isolation import LimitsWriter
from elastic_gpu_agent_amd.operator import GPUOperator, unlink_many
from elastic_gpu_agent_amd.operator.fake import FakeBackend
from elastic_gpu_agent_amd.types import Device, PodContainer
from helpers import Harness

_fastwire = pytest.importorskip("elastic_gpu_agent_amd._fastwire")


def py_make_links(pairs):
    for target, link in pairs:
        GPUOperator._force_symlink(target, link)


MAKERS = [pytest.param(py_make_links, id="python"),
          pytest.param(lambda pairs: _fastwire.make_links(pairs), id="native")]


# ---- make_links ---------------------------------------------------------------

@pytest.mark.parametrize("make_links", MAKERS)
def test_links_fresh_correct_wrong_and_file_in_the_way(tmp_path, make_links):
    gpu, ctl = str(tmp_path / "elastic-gpu-x-0"), str(tmp_path / "elastic-gpuctl-x-0")
    pairs = [("/dev/dri/renderD128", gpu), ("/dev/kfd", ctl)]
    make_links(pairs)  # fresh
    assert (os.readlink(gpu), os.readlink(ctl)) == ("/dev/dri/renderD128", "/dev/kfd")
    ino = os.lstat(gpu).st_ino
    make_links(pairs)  # already correct: left alone
    assert os.lstat(gpu).st_ino == ino
    os.unlink(gpu)
    os.symlink("/dev/dri/renderD129", gpu)  # wrong target
    os.unlink(ctl)
    with open(ctl, "w") as f:  # a regular file in the way
        f.write("x")
    make_links(pairs)
    assert (os.readlink(gpu), os.readlink(ctl)) == ("/dev/dri/renderD128", "/dev/kfd")
    # a target that only starts with the wanted one is wrong too
    os.unlink(ctl)
    os.symlink("/dev/kfd2", ctl)
    make_links(pairs)
    assert os.readlink(ctl) == "/dev/kfd"


@pytest.mark.parametrize("make_links", MAKERS)
def test_links_missing_directory_is_enoent(tmp_path, make_links):
    with pytest.raises(OSError) as ei:
        make_links([("/dev/kfd", str(tmp_path / "gone" / "link"))])
    assert ei.value.errno == errno.ENOENT
    assert isinstance(ei.value, FileNotFoundError)


def test_create_makes_dev_root_once_and_again_when_it_is_gone(tmp_path):
    root = tmp_path / "dev"
    op = GPUOperator(FakeBackend(count=1), dev_root=str(root))
    op.create(0, "aaaa-0")
    assert op.check(0, "aaaa-0")
    for name in os.listdir(root):
        os.unlink(root / name)
    os.rmdir(root)
    op.create(0, "bbbb-0")  # ENOENT: the directory is made again, one retry
    assert op.check(0, "bbbb-0")
    minor = op.device_by_index(0).drm_render_minor
    assert os.readlink(root / "elastic-gpu-bbbb-0") == consts.DRI_RENDER_FMT % minor
    assert os.readlink(root / "elastic-gpuctl-bbbb-0") == consts.KFD_PATH


# ---- atomic_write -------------------------------------------------------------

REC = {"version": 1, "gpu_indexes": [0], "render_minors": [128], "uuids": ["GPU-é\"\\"],
       "cu_mask": "0xffff", "cu_count": 16, "mem_limit_bytes": 1 << 34,
       "priority": None}


def json_dump_bytes(obj):
    buf = io.StringIO()
    json.dump(obj, buf)
    return buf.getvalue().encode()


def tmp_files(d):
    return [n for n in os.listdir(d) if n.endswith(".tmp")]


def test_atomic_write_bytes_mode_and_no_temp_left(tmp_path):
    path = str(tmp_path / "abcd1234.json")
    LimitsWriter._atomic_write(path, REC)
    with open(path, "rb") as f:
        assert f.read() == json_dump_bytes(REC)
    assert stat.S_IMODE(os.stat(path).st_mode) == 0o600  # as mkstemp's
    assert tmp_files(tmp_path) == []
    _fastwire.atomic_write(path, b"")  # replaces; an empty payload is fine
    assert os.path.getsize(path) == 0
    assert os.listdir(tmp_path) == ["abcd1234.json"]


def test_atomic_write_failure_leaves_no_temp(tmp_path):
    blocker = tmp_path / "file"
    blocker.write_text("x")
    with pytest.raises(OSError) as ei:  # the parent path is a file
        _fastwire.atomic_write(str(blocker / "x.json"), b"{}")
    assert ei.value.errno == errno.ENOTDIR
    # the rename is what fails here: the written temp file must go
    target = tmp_path / "dir.json"
    (target / "sub").mkdir(parents=True)
    with pytest.raises(OSError) as ei:
        _fastwire.atomic_write(str(target), b"{}")
    assert ei.value.errno in (errno.EISDIR, errno.ENOTEMPTY, errno.EEXIST)
    assert tmp_files(tmp_path) == []
    assert sorted(os.listdir(tmp_path)) == ["dir.json", "file"]


@pytest.fixture
def mem_dir(tmp_path):
    """A directory on a memory-backed filesystem where there is one: a rename
    over an existing file makes ext4 write the new file's data out first, so
    400 of them can take a disk many seconds."""
    import shutil
    import tempfile

    if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK | os.X_OK):
        d = tempfile.mkdtemp(prefix="egpu-bindfx-", dir="/dev/shm")
        try:
            yield pathlib.Path(d)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    else:
        yield tmp_path


def test_atomic_write_threads_leave_one_whole_payload(mem_dir):
    tmp_path = mem_dir
    path = str(tmp_path / "shared.json")
    payloads = [json.dumps({"writer": t, "pad": "x" * (200 + 37 * t)}).encode()
                for t in range(8)]
    errors = []

    def writer(t):
        try:
            for _ in range(50):
                _fastwire.atomic_write(path, payloads[t])
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=writer, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    with open(path, "rb") as f:
        assert f.read() in payloads
    assert os.listdir(tmp_path) == ["shared.json"]


# ---- unlink_many ---------------------------------------------------------------

@pytest.mark.parametrize("native", [False, True], ids=["python", "native"])
def test_unlink_many_with_missing_entries(tmp_path, monkeypatch, native):
    import elastic_gpu_agent_amd.operator as operator_mod

    if not native:
        monkeypatch.setattr(operator_mod, "_native_unlink_many", None)
    keep = tmp_path / "keep"
    keep.write_text("k")
    paths = []
    for i in range(4):
        p = tmp_path / f"f{i}"
        p.write_text("x")
        paths.append(str(p))
    os.symlink("/dev/kfd", tmp_path / "l")
    paths.insert(1, str(tmp_path / "missing"))
    paths.append(str(tmp_path / "l"))
    paths.append(str(tmp_path / "nodir" / "missing"))
    unlink_many(paths)
    assert os.listdir(tmp_path) == ["keep"]
    unlink_many(paths)  # all missing now
    unlink_many([])
    # a directory cannot be unlinked: raised, but only after the rest went
    d = tmp_path / "d"
    d.mkdir()
    keep2 = tmp_path / "after"
    keep2.write_text("x")
    with pytest.raises(OSError) as ei:
        unlink_many([str(d), str(keep2)])
    assert ei.value.errno in (errno.EISDIR, errno.EPERM)
    assert ei.value.filename == str(d)
    assert sorted(os.listdir(tmp_path)) == ["d", "keep"]


# ---- a bind, then GC ------------------------------------------------------------

def test_bind_then_gc_leaves_the_directories_empty(tmp_path):
    h = Harness(str(tmp_path))
    h.paths.state_dir = str(tmp_path / "state")  # the default is under /host
    try:
        ids =[f"0-{i:02d}" for i in range(25)]
        d = Device.new(ids, consts.RESOURCE_GPU_CORE)
        h.core_locator.assign(d.hash, PodContainer("ns", "p", "main"))
        h.add_assumed_pod("ns", "p", "main", "0")
        h.plugin.core.allocate({"container_requests": [{"devicesIDs": ids}]}, None)
        h.plugin.core.pre_start_container({"devicesIDs": ids}, None)
        pids = os.path.join(h.paths.state_dir, "pids")
        os.makedirs(pids, exist_ok=True)
        with open(os.path.join(pids, d.hash), "w") as f:
            f.write("1234\n")
        assert sorted(os.listdir(h.paths.dev_root)) == [
            f"elastic-gpu-{d.hash}-0", f"elastic-gpuctl-{d.hash}-0"]
        assert os.listdir(h.paths.limits_dir) == [f"{d.hash}.json"]
        assert h.plugin.cfg.limits.read(d.hash)["gpu_indexes"] == [0]
        h.sitter.remove("ns", "p")
        assert h.plugin.gc_once() == 1
        assert os.listdir(h.paths.dev_root) == []
        assert os.listdir(h.paths.limits_dir) == []
        assert os.listdir(pids) == []
    finally:
        h.close()
