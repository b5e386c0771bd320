"""Flagship benchmark: fractional-pod churn against the device-plugin stack.

Measures the BASELINE.json metric — "fractional pods/GPU + p50 Allocate() RPC
latency at 1/2/4/8 MI355X" — by driving the full agent pipeline over real
gRPC unix sockets in the PRODUCTION SHAPE: **one agent per node managing all
N GPUs** (the reference runs as a DaemonSet, one pod per node —
deploy/elastic-gpu-agent.yaml:78-87), with one load-generator rank per GPU:

  rank 0   hosts the single agent (all N GPUs, one storage, one CU-mask
           allocator, both resource servers) and simulates the kubelet-side
           bookkeeping (podresources assignment + pod annotations);
  rank r   drives GPU r's pods over the shared unix sockets: Allocate +
           PreStartContainer per pod [the timed RPCs].

  step = assign+annotate all pods (rank 0) → barrier → every rank binds its
         GPU's pods concurrently → barrier → rank 0 deletes the pods and
         runs one GC reconciliation pass.

`--agent-mode per-gpu` keeps the round-1 shape (N independent agents) for
comparison. The kubelet side is simulated in-process; the GPU side is real
when available (libamd_smi enumeration; PreStart materializes symlinks to
the node's actual /dev/dri/renderD* minors).

Output: ONE JSON line on rank 0 (driver contract), value = whole-job pod
allocation-cycle throughput (cycles/s over all ranks), plus worst-rank
p50/p99 Allocate RPC latency in µs. The memory unit defaults to the
reference-exact 1 MiB contract (294,912 device IDs per 288 GB GPU).

Configs (--config): mixed (default; core fractions + memory fractions, 16
pods/GPU oversubscribed), whole-gpu, mem-fraction, compute-fraction,
kind-fake (forces the fake backend).

A plain run does only what the headline needs: set up, warm up, time
--steps steps, print the line. `--dump-outputs DIR` additionally saves what
the last timed step produced (see dump_outputs). `--full` is where any
measurement beyond the headline belongs (baselines, other scenarios,
per-stage attribution); the benchmark has none today — other scenarios and
agent shapes are separate invocations via --config / --agent-mode /
--workers — so the flag is accepted and changes nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def get_dist():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, world


def pod_plan(config: str, pods_per_gpu: int, gpu_index: int, mem_total_mib: int,
             mem_unit_mib: int):
    """Returns a list of (kind, ids) per pod for one GPU."""
    plans = []
    if config == "whole-gpu":
        plans.append(("core", [f"{gpu_index}-{i:02d}" for i in range(100)]))
        return plans
    if config == "mem-fraction":
        # 4 pods × 1/4 of HBM (the 72 GiB config on 288 GB parts)
        units = mem_total_mib // mem_unit_mib // 4
        for p in range(4):
            plans.append(
                ("mem", [f"{gpu_index}-{p * units + i:06d}" for i in range(units)])
            )
        return plans
    if config == "compute-fraction":
        # 8 pods × 12% of the card (CU-mask partitions)
        for p in range(8):
            plans.append(("core", [f"{gpu_index}-{(p * 12 + i) % 100:02d}" for i in range(12)]))
        return plans
    # mixed (default): pods_per_gpu pods alternating core fractions and
    # memory fractions, oversubscribed core (sum > 100%)
    for p in range(pods_per_gpu):
        if p % 2 == 0:
            frac = 10 + (p % 5) * 5
            start = (p * 7) % 90
            plans.append(
                ("core", [f"{gpu_index}-{(start + i) % 100:02d}" for i in range(frac)])
            )
        else:
            units = max(1, mem_total_mib // mem_unit_mib // max(pods_per_gpu, 1))
            base = (p // 2) * units
            plans.append(("mem", [f"{gpu_index}-{base + i:06d}" for i in range(units)]))
    return plans


def pick_backend(config: str):
    import torch

    if config != "kind-fake" and torch.cuda.is_available():
        try:
            from elastic_gpu_agent_amd.operator.amdsmi import AmdSmiBackend

            backend = AmdSmiBackend()
            backend.devices()
            return backend, "amdsmi"
        except Exception as e:
            print(f"# amdsmi backend unavailable ({e}); using fake", file=sys.stderr)
    return None, "fake-gfx950"


def install_backend(h, backend):
    if backend is None:
        return
    from elastic_gpu_agent_amd.isolation import CUMaskAllocator
    from elastic_gpu_agent_amd.operator import GPUOperator

    h.plugin.cfg.operator = GPUOperator(backend, dev_root=h.paths.dev_root)
    h.plugin.cfg.cumask = CUMaskAllocator(
        h.storage, backend.devices(),
        on_remask=lambda hh, m, n: h.plugin.cfg.limits.update_in_place(
            hh, cu_mask=m, cu_count=n))


def response_rows(responses, root):
    """One row per pod from its decoded AllocateResponse: device-set hash,
    env / device / mount counts, and a CRC32 of the whole response with the
    per-run scratch root masked out (equal responses give equal rows)."""
    import zlib

    from elastic_gpu_agent_amd import consts

    rows = []
    for resp in responses:
        cr = resp["container_responses"][0]
        canon = json.dumps(resp, sort_keys=True).replace(root, "<root>")
        rows.append([int(cr["envs"][consts.GPU_ENV_KEY], 16),
                     len(cr.get("envs", {})), len(cr.get("devices", [])),
                     len(cr.get("mounts", [])), zlib.crc32(canon.encode())])
    return rows


def binding_rows(limits, hashes):
    """One row per bound pod from the limits file PreStart wrote for it:
    device-set hash, GPU index, number of render nodes bound (the minor
    itself names the card, not the computation), CU count and HBM quota (0 =
    unlimited), then the CU mask as 32-bit words."""
    from elastic_gpu_agent_amd.isolation.cumask import parse_mask_hex

    recs = [limits.read(h) for h in hashes]
    masks = [parse_mask_hex(r.get("cu_mask", "")) for r in recs]
    width = max((len(m) for m in masks), default=0)
    rows = []
    for h, r, m in zip(hashes, recs, masks):
        rows.append([int(h, 16), r["gpu_indexes"][0],
                     len(r.get("render_minors", [])),
                     r.get("cu_count", 0), r.get("mem_limit_bytes", 0)]
                    + m + [0] * (width - len(m)))
    return rows


def dump_outputs(out_dir, responses, bindings):
    """--dump-outputs: what a caller of the timed path holds after the LAST
    timed step, as float64 arrays (every value is an integer < 2**53, so
    exact). Inputs are fixed by the arguments, so two builds run with the
    same arguments can be compared array for array.

      allocate_responses.npy  [pods, 5]     response_rows() of rank 0's pods
      bindings.npy            [pods, 5+W]   binding_rows() of every rank's
                                            pods, read after PreStart and
                                            before the step's teardown
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "allocate_responses.npy"),
            np.asarray(responses, dtype=np.float64))
    np.save(os.path.join(out_dir, "bindings.npy"),
            np.asarray(bindings, dtype=np.float64))


def emit(rank, value, elapsed_max, args, world, n_gpus, pods_per_step_job,
         p50_us, p99_us, p50_prestart_us, backend_name, mode_str):
    if rank != 0:
        return
    print(json.dumps({
        "metric": "fractional pods/GPU + p50 Allocate() RPC latency at 1/2/4/8 MI355X",
        "value": round(value, 2),
        "unit": "pod-allocation-cycles/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed_max / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "n/a",
        "data": "synthetic",
        "p50_allocate_us": round(p50_us, 1),
        "p99_allocate_us": round(p99_us, 1),
        "p50_prestart_us": round(p50_prestart_us, 1),
        "config": {
            "model": "gpushare-device-plugin",
            "scenario": args.config,
            "pods_per_gpu": pods_per_step_job // max(world, 1),
            "backend": backend_name,
            "mem_unit_mib": args.mem_unit_mib,
            "global_batch": pods_per_step_job,
            "seq_len": 0,
            "parallelism": mode_str,
        },
    }))


def reduce_stats(dist, torch, elapsed, alloc_lat, prestart_lat):
    lat_sorted = sorted(alloc_lat) or [0.0]
    p50_us = lat_sorted[len(lat_sorted) // 2] * 1e6
    p99_us = lat_sorted[min(len(lat_sorted) - 1, int(0.99 * len(lat_sorted)))] * 1e6
    ps_sorted = sorted(prestart_lat) or [0.0]
    p50_prestart_us = ps_sorted[len(ps_sorted) // 2] * 1e6
    elapsed_max = elapsed
    if dist is not None:
        t = torch.tensor([elapsed, p50_us, p99_us, p50_prestart_us])
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_max, p50_us, p99_us, p50_prestart_us = (float(x) for x in t)
    return elapsed_max, p50_us, p99_us, p50_prestart_us


def _spawn_agent_workers(tmp, n_gpus, args, backend_name):
    """Bind the two plugin sockets and launch --workers pre-forked agent
    processes accepting on them (pass_fds). Returns (paths, procs)."""
    import socket
    import subprocess

    core_path = os.path.join(tmp, "core.sock")
    mem_path = os.path.join(tmp, "mem.sock")
    fds = []
    for path in (core_path, mem_path):
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        s.bind(path)
        s.listen(512)
        s.set_inheritable(True)
        fds.append(s)
    procs = []
    for w in range(args.workers):
        ready = os.path.join(tmp, f"worker-{w}.ready")
        p = subprocess.Popen(
            [sys.executable, os.path.join(REPO, "tests", "bench_worker.py"),
             tmp, str(n_gpus), str(args.mem_unit_mib),
             str(fds[0].fileno()), str(fds[1].fileno()), backend_name, ready],
            pass_fds=(fds[0].fileno(), fds[1].fileno()), cwd=REPO,
        )
        procs.append((p, ready))
    deadline = time.time() + 120
    for p, ready in procs:
        while not os.path.exists(ready):
            if p.poll() is not None:
                raise RuntimeError(f"agent worker died rc={p.returncode}")
            if time.time() > deadline:
                raise RuntimeError("agent workers never became ready")
            time.sleep(0.05)
    return core_path, mem_path, fds, [p for p, _ in procs]


def run_single_agent(args, rank, world, dist):
    """Production shape: ONE agent (rank 0) manages all N GPUs; every rank
    is a load generator for one GPU. With --workers > 0 the agent's data
    plane is pre-forked: N worker processes accept on the same listening
    sockets (kernel load-balancing), coordinating through the shared state
    DB (sqlite WAL) and filesystem — the CPython GIL caps a single process
    at ~1 core of handler throughput, so thread-level concurrency cannot
    scale a one-process agent (measured 0.6-0.8× at 4 threads)."""
    import torch

    from elastic_gpu_agent_amd import consts
    from elastic_gpu_agent_amd.types import Device, PodContainer
    from helpers import Harness, PluginClient, short_tmpdir

    backend, backend_name = (None, "fake-gfx950")
    h = None
    worker_procs = []
    listen_socks = []
    if rank == 0:
        backend, backend_name = pick_backend(args.config)
        tmp = short_tmpdir("egpu-bench-agent-")
        # fake-backend GPU count (EGPU_BENCH_GPUS lets tests model fewer
        # GPUs than ranks — the shape a 1-GPU box gives a multi-rank run)
        n_fake = int(os.environ.get("EGPU_BENCH_GPUS", world))
        if args.workers > 0:
            from helpers import build_worker_harness

            # parent-side stack: kubelet bookkeeping + GC (never serves)
            plugin, storage = build_worker_harness(
                tmp, n_fake, args.mem_unit_mib, backend=backend)

            class _H:  # minimal Harness-shaped view for the shared paths
                pass

            h = _H()
            h.plugin = plugin
            h.storage = storage
            h.sitter = plugin.cfg.sitter
            h.core_locator = plugin.cfg.core_locator
            h.mem_locator = plugin.cfg.memory_locator

            def _add_assumed(ns, name, container, gpu_indexes, _s=h.sitter):
                from elastic_gpu_agent_amd.kube.pods import Pod

                _s.add(Pod(namespace=ns, name=name, annotations={
                    consts.ELASTIC_GPU_ASSUMED_ANNOTATION: "true",
                    consts.ELASTIC_GPU_CONTAINER_ANNOTATION % container: gpu_indexes,
                }))

            h.add_assumed_pod = _add_assumed

            def _close(plugin=plugin, storage=storage):
                plugin.stop()
                storage.close()

            h.close = _close
            core_sock_path, mem_sock_path, listen_socks, worker_procs = \
                _spawn_agent_workers(tmp, n_fake, args, backend_name)
        else:
            h = Harness(tmp, gpus=n_fake, mem_unit_mib=args.mem_unit_mib)
            install_backend(h, backend)
            h.plugin.core_server.serve()
            h.plugin.memory_server.serve()
            h.plugin.core_server.wait_ready()
            h.plugin.memory_server.wait_ready()
            core_sock_path = h.plugin.core_server.socket_path
            mem_sock_path = h.plugin.memory_server.socket_path
        gpus = h.plugin.cfg.operator.devices()
        shared = [core_sock_path, mem_sock_path,
                  [(g.index, g.memory_mib) for g in gpus],
                  backend_name]
    else:
        shared = [None, None, None, None]
    if dist is not None:
        dist.broadcast_object_list(shared, src=0)
    core_sock, mem_sock, gpu_list, backend_name = shared

    # rank r drives GPU r (mod available — a 1-GPU box still runs any world).
    # Device-ID sets are prefixed by RANK, not GPU: ids are opaque to the
    # binding path (the GPU comes from the pod annotation), and kubelet
    # never assigns the same fake ID to two live pods — two ranks sharing a
    # physical GPU must not collide on device-set hashes.
    my_gpu_index, my_mem_mib = gpu_list[rank % len(gpu_list)]
    plans = pod_plan(args.config, args.pods_per_gpu, rank, my_mem_mib,
                     args.mem_unit_mib)
    pods_per_step = len(plans)

    core = PluginClient(core_sock)
    mem = PluginClient(mem_sock)

    # Pre-encode each pod's request bytes once (the ID sets repeat every
    # step): the load generator plays kubelet, and a real kubelet holds its
    # device lists in wire-ready form — request serialization is client-side
    # work, not agent latency. The timed window still covers the full RPC:
    # transport, digest, handler, persistence, response.
    from elastic_gpu_agent_amd.protos import fastpath

    encoded_plans = [
        (kind,
         fastpath.encode_allocate_request(
             {"container_requests": [{"devicesIDs": ids}]}),
         fastpath.encode_prestart_request({"devicesIDs": ids}))
        for kind, ids in plans
    ]

    alloc_lat, prestart_lat = [], []
    # --dump-outputs: each pod's latest AllocateResponse (overwritten every
    # step) and, from the last timed step, the bindings PreStart left
    last_responses = [None] * len(encoded_plans)
    last_bindings = []

    # Precompute every (rank, pod) device hash once: the ID sets repeat
    # every step (only the pod name changes), and the kubelet stand-in must
    # not spend milliseconds re-hashing 73k-ID sets inside the timed region.
    all_plans = []
    if rank == 0:
        for r in range(world):
            g_idx, g_mem = gpu_list[r % len(gpu_list)]
            # ids prefixed by rank (unique across ranks sharing a GPU);
            # the ANNOTATION carries the physical GPU index
            for p, (kind, ids) in enumerate(
                    pod_plan(args.config, args.pods_per_gpu, r, g_mem,
                             args.mem_unit_mib)):
                res = (consts.RESOURCE_GPU_CORE if kind == "core"
                       else consts.RESOURCE_GPU_MEMORY)
                d = Device.new(ids, res)
                all_plans.append((r, p, kind, d.hash, str(g_idx)))

    def setup_step(step_i: int):
        """Rank 0: kubelet-side bookkeeping for EVERY rank's pods."""
        for r, p, kind, dhash, g_idx in all_plans:
            ns, name, container = "bench", f"pod-{step_i}-r{r}-{p}", "main"
            locator = h.core_locator if kind == "core" else h.mem_locator
            locator.assign(dhash, PodContainer(ns, name, container))
            h.add_assumed_pod(ns, name, container, g_idx)

    def drive_step(step_i: int):
        """Every rank: bind its GPU's pods over the wire."""
        for p, (kind, alloc_raw, pre_raw) in enumerate(encoded_plans):
            client = core if kind == "core" else mem
            t0 = time.perf_counter()
            last_responses[p] = client.allocate_raw(alloc_raw)
            t1 = time.perf_counter()
            client.pre_start_raw(pre_raw)
            t2 = time.perf_counter()
            alloc_lat.append(t1 - t0)
            prestart_lat.append(t2 - t1)

    def teardown_step(step_i: int):
        for r in range(world):
            for p in range(pods_per_step):
                h.sitter.remove("bench", f"pod-{step_i}-r{r}-{p}")
        reclaimed = h.plugin.gc_once()
        want = world * pods_per_step
        assert reclaimed == want, f"GC reclaimed {reclaimed}/{want}"

    def barrier():
        if dist is not None:
            dist.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def one_step(step_i: int):
        if rank == 0:
            setup_step(step_i)
        barrier()
        drive_step(step_i)
        barrier()
        if rank == 0:
            if args.dump_outputs and step_i == args.steps - 1:
                last_bindings.extend(binding_rows(
                    h.plugin.cfg.limits, [pl[3] for pl in all_plans]))
            teardown_step(step_i)

    for w in range(args.warmup):
        one_step(-1 - w)

    alloc_lat.clear()
    prestart_lat.clear()
    barrier()
    t_start = time.perf_counter()
    for s in range(args.steps):
        one_step(s)
    barrier()
    elapsed = time.perf_counter() - t_start

    elapsed_max, p50_us, p99_us, p50_pre = reduce_stats(
        dist, torch, elapsed, alloc_lat, prestart_lat)
    pods_job = world * pods_per_step
    value = pods_job * args.steps / elapsed_max

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, response_rows(last_responses, tmp),
                     last_bindings)

    core.close()
    mem.close()
    for p in worker_procs:
        p.terminate()
    for p in worker_procs:
        try:
            p.wait(timeout=10)
        except Exception:
            p.kill()
    for s in listen_socks:
        s.close()
    if h is not None:
        h.close()
        shutil.rmtree(tmp, ignore_errors=True)
    mode =(f"1 agent x {world} GPUs ({world} load ranks, "
            f"{args.workers} workers)" if args.workers > 0
            else f"1 agent x {world} GPUs ({world} load ranks)")
    emit(rank, value, elapsed_max, args, world, len(gpu_list), pods_job,
         p50_us, p99_us, p50_pre, backend_name, mode)


def run_per_gpu(args, rank, world, dist):
    """Round-1 comparison shape: N independent agents, one per GPU."""
    import torch

    from elastic_gpu_agent_amd import consts
    from elastic_gpu_agent_amd.types import Device, PodContainer
    from helpers import Harness, PluginClient, short_tmpdir

    backend, backend_name = pick_backend(args.config)
    tmp = short_tmpdir(f"egpu-bench-r{rank}-")
    h = Harness(tmp, gpus=1, mem_unit_mib=args.mem_unit_mib)
    install_backend(h, backend)
    gpus = h.plugin.cfg.operator.devices()
    gpu = gpus[min(rank, len(gpus) - 1)]

    h.plugin.core_server.serve()
    h.plugin.memory_server.serve()
    h.plugin.core_server.wait_ready()
    h.plugin.memory_server.wait_ready()
    core = PluginClient(h.plugin.core_server.socket_path)
    mem = PluginClient(h.plugin.memory_server.socket_path)

    plans = pod_plan(args.config, args.pods_per_gpu, gpu.index, gpu.memory_mib,
                     args.mem_unit_mib)
    pods_per_step = len(plans)
    alloc_lat, prestart_lat = [], []
    last_responses = [None] * len(plans)  # --dump-outputs, as in single mode
    last_bindings = []

    def one_step(step_i: int):
        pods = []
        for p, (kind, ids) in enumerate(plans):
            ns, name, container = "bench", f"pod-{step_i}-{p}", "main"
            res = consts.RESOURCE_GPU_CORE if kind == "core" else consts.RESOURCE_GPU_MEMORY
            d = Device.new(ids, res)
            locator = h.core_locator if kind == "core" else h.mem_locator
            locator.assign(d.hash, PodContainer(ns, name, container))
            h.add_assumed_pod(ns, name, container, str(gpu.index))
            client = core if kind == "core" else mem
            t0 = time.perf_counter()
            last_responses[p] = client.allocate(
                {"container_requests": [{"devicesIDs": ids}]})
            t1 = time.perf_counter()
            client.pre_start({"devicesIDs": ids})
            t2 = time.perf_counter()
            alloc_lat.append(t1 - t0)
            prestart_lat.append(t2 - t1)
            pods.append((ns, name, d))
        if rank == 0 and args.dump_outputs and step_i == args.steps - 1:
            last_bindings.extend(binding_rows(
                h.plugin.cfg.limits, [d.hash for _, _, d in pods]))
        for ns, name, _ in pods:
            h.sitter.remove(ns, name)
        reclaimed = h.plugin.gc_once()
        assert reclaimed == len(pods), f"GC reclaimed {reclaimed}/{len(pods)}"

    def barrier():
        if dist is not None:
            dist.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    for w in range(args.warmup):
        one_step(-1 - w)
    alloc_lat.clear()
    prestart_lat.clear()
    barrier()
    t_start = time.perf_counter()
    for s in range(args.steps):
        one_step(s)
    barrier()
    elapsed = time.perf_counter() - t_start

    elapsed_max, p50_us, p99_us, p50_pre = reduce_stats(
        dist, torch, elapsed, alloc_lat, prestart_lat)
    value = world * pods_per_step * args.steps / elapsed_max
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, response_rows(last_responses, tmp),
                     last_bindings)
    core.close()
    mem.close()
    h.close()
    shutil.rmtree(tmp, ignore_errors=True)
    emit(rank, value, elapsed_max, args, world, world, world * pods_per_step,
         p50_us, p99_us, p50_pre, backend_name,
         f"dp{world} (1 agent per GPU)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pods-per-gpu", type=int, default=16)
    ap.add_argument("--config", default="mixed",
                    choices=["mixed", "whole-gpu", "mem-fraction", "compute-fraction",
                             "kind-fake"])
    # 1 MiB is the reference-exact contract unit (pkg/plugins/gpushare.go:161
    # with pkg/operator/base.go:35-39) — the headline runs at the contract
    ap.add_argument("--mem-unit-mib", type=int, default=1)
    ap.add_argument("--agent-mode", default="single", choices=["single", "per-gpu"],
                    help="single = production shape (one agent, N GPUs); "
                         "per-gpu = N independent agents (round-1 shape)")
    ap.add_argument("--workers", type=int, default=0,
                    help="single mode: pre-forked agent data-plane processes "
                         "accepting on the shared sockets (0 = in-process, "
                         "the measured-fastest default; >0 trades GIL-bound "
                         "handler concurrency for cross-process state "
                         "coordination — wins when handlers dominate, loses "
                         "when the shared single-file store does)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, save what the last one "
                         "produced as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline figure "
                         "(none exist today; a plain run is already complete)")
    args = ap.parse_args()

    rank, world = get_dist()
    dist = None
    if world > 1:
        import torch.distributed as tdist

        tdist.init_process_group(backend="gloo")
        dist = tdist

    if args.agent_mode == "single":
        run_single_agent(args, rank, world, dist)
    else:
        run_per_gpu(args, rank, world, dist)

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
