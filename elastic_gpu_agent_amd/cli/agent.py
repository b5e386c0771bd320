"""Agent entrypoint (DaemonSet container).

Flags mirror the reference's (ref: cmd/main.go:17-35) plus MI355X options.
SIGUSR1 dumps all thread stacks (the reference's goroutine-dump equivalent,
ref: pkg/common/util.go:58-66) via faulthandler.
"""
from __future__ import annotations

import argparse
import faulthandler
import logging
import signal
import sys
import threading


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(prog="elastic-gpu-agent-amd")
    parser.add_argument("--nodeName", "-nodeName", default="", help="node this agent runs on")
    parser.add_argument(
        "--dbFile", "-dbFile", default="/host/var/lib/egpu/meta.db", help="allocation state DB"
    )
    parser.add_argument("--kubeconf", "-kubeconf", default=None, help="kubeconfig path")
    parser.add_argument(
        "--gpuPluginName", "-gpuPluginName", default="gpushare", help="plugin to run"
    )
    parser.add_argument(
        "--backend", default="amdsmi", choices=["amdsmi", "fake"],
        help="GPU enumeration backend (fake = synthetic gfx950 fleet)",
    )
    parser.add_argument(
        "--mem-unit-mib", type=int, default=1,
        help="MiB of HBM per gpu-memory unit (1 = reference contract; "
        "1024 recommended for 288 GB parts if kubelet device counts bite)",
    )
    parser.add_argument(
        "--no-isolation", action="store_true",
        help="disable HSA-shim CU-mask/HBM-quota injection",
    )
    parser.add_argument("--metrics-port", type=int, default=0, help="Prometheus port (0=off)")
    parser.add_argument("--workers", type=int, default=0,
                        help="pre-forked data-plane worker processes accepting "
                             "on the plugin sockets (0 = serve in-process)")
    parser.add_argument("--gpu-selftest-seconds", type=float, default=0.0,
                        help="run the active GPU self-test on every GPU this "
                             "often; a failing GPU is advertised Unhealthy "
                             "until `egpuctl health IDX --clear` (0 = off)")
    parser.add_argument("--gpu-selftest-timeout", type=float, default=10.0,
                        help="time limit of one self-test probe; a probe that "
                             "exceeds it makes its GPU Unhealthy")
    parser.add_argument("--gpu-selftest-matrix", action="store_true",
                        help="each self-test probe also runs the matrix sweep: "
                             "the FP8, FP6, FP4, INT8, F16 and 16x16 MFMA paths")
    parser.add_argument("--recordFormat", choices=["runs", "list"], default="runs",
                        help="how the state DB holds a large consecutive device "
                             "set: as ID runs, or as the literal list that "
                             "builds before the runs form read (use list "
                             "before rolling back to such a build)")
    parser.add_argument("--hashMemoEntries", type=int, default=256,
                        help="device sets whose hash Allocate keeps for the "
                             "PreStart that follows, so a large set is hashed "
                             "once per bind instead of twice (0 = off)")
    # path overrides (defaults match the DaemonSet mounts; overridable for
    # local runs and tests)
    parser.add_argument("--plugin-dir", default=None, help="kubelet device-plugins dir")
    parser.add_argument("--podresources-socket", default=None)
    parser.add_argument("--dev-root", default=None, help="host /dev mount")
    parser.add_argument("--limits-dir", default=None)
    parser.add_argument("--state-dir", default=None)
    parser.add_argument("--shim-host-path", default=None)
    parser.add_argument("-v", "--verbose", action="count", default=0)
    args = parser.parse_args(argv)

    logging.basicConfig(
        level=logging.DEBUG if args.verbose else logging.INFO,
        format="%(asctime)s %(levelname)s %(name)s: %(message)s",
    )
    # httpx logs one INFO line per API request — at GC/watch volume that is
    # pure noise (and measurable I/O); our own loggers cover the decisions
    if not args.verbose:
        logging.getLogger("httpx").setLevel(logging.WARNING)
    faulthandler.register(signal.SIGUSR1, all_threads=True)

    from ..manager import GPUManager, ManagerOptions
    from ..plugins.config import AgentPaths, PluginOptions

    paths = AgentPaths()
    if args.plugin_dir:
        paths.plugin_dir = args.plugin_dir
        paths.kubelet_socket = None  # re-derive from plugin_dir
    if args.podresources_socket:
        paths.podresources_socket = args.podresources_socket
    if args.dev_root:
        paths.dev_root = args.dev_root
    if args.limits_dir:
        paths.limits_dir = args.limits_dir
    if args.state_dir:
        paths.state_dir = args.state_dir
    if args.shim_host_path:
        paths.shim_host_path = args.shim_host_path

    opts = ManagerOptions(
        node_name=args.nodeName,
        db_path=args.dbFile,
        kubeconf=args.kubeconf,
        gpu_plugin_name=args.gpuPluginName,
        backend=args.backend,
        paths=paths,
        plugin_options=PluginOptions(
            mem_unit_mib=args.mem_unit_mib, isolation=not args.no_isolation
        ),
        metrics_port=args.metrics_port,
        workers=args.workers,
        selftest_seconds=args.gpu_selftest_seconds,
        selftest_timeout=args.gpu_selftest_timeout,
        selftest_matrix=args.gpu_selftest_matrix,
        record_format=args.recordFormat,
        hash_memo_entries=args.hashMemoEntries,
    )
    manager = GPUManager(opts)
    manager.run()

    stop = threading.Event()

    def _term(signum, frame):
        stop.set()

    signal.signal(signal.SIGTERM, _term)
    signal.signal(signal.SIGINT, _term)
    stop.wait()
    try:
        manager.stop()
    except Exception:  # a teardown race must not turn TERM into rc!=0
        import traceback

        traceback.print_exc()
    return 0


if __name__ == "__main__":
    sys.exit(main())
