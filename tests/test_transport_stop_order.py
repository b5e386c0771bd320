"""A plugin server can be stopped from another thread while its own thread is
still bringing it up (BasePluginServer.serve() binds and starts; stop() may
land in between). The native ServerCore must then stay inert: no accept
thread is created after stop(), so dropping the object is clean."""
import gc
import os

import pytest

_etransport = pytest.importorskip("elastic_gpu_agent_amd._etransport")


def test_start_after_stop_creates_nothing(tmp_path):
    path = str(tmp_path / "s.sock")
    core = _etransport.ServerCore()
    core.bind_unix(path)
    core.stop()
    assert not os.path.exists(path)
    core.start()  # lost the race against stop(): must be a no-op
    core.stop()
    del core
    gc.collect()


def test_dropped_without_stop_joins_its_accept_thread(tmp_path):
    path = str(tmp_path / "s.sock")
    core = _etransport.ServerCore()
    core.bind_unix(path)
    core.start()
    core.start()  # a second start does not replace the running thread
    del core
    gc.collect()
