import pathlib
import shutil

import pytest


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: test requires a real MI355X (gfx950) GPU")


@pytest.fixture
def tmp_path(tmp_path):
    """pytest's tmp_path, unless it is too long to hold the agent's unix
    sockets (sun_path is 107 bytes; a nested $TMPDIR plus pytest's own
    pytest-of-<user>/pytest-N/<test name> levels overflow it) — then a short
    directory that is removed after the test."""
    from helpers import SOCKET_ROOT_MAX, short_tmpdir

    if len(str(tmp_path)) <= SOCKET_ROOT_MAX:
        yield tmp_path
        return
    short = short_tmpdir("egpu-t-")
    try:
        yield pathlib.Path(short)
    finally:
        shutil.rmtree(short, ignore_errors=True)


@pytest.fixture
def tmp_db(tmp_path):
    return str(tmp_path / "meta.db")
