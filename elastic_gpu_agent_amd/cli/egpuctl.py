"""egpuctl — node-local admin CLI for the MI355X elastic-gpu agent.

Subcommands:
  devices                 enumerate GPUs (amdsmi or --fake)
  pods                    list persisted allocations
  masks                   list live CU-mask assignments
  occupancy               per-pod live occupancy (amdsmi join)
  partition IDX [MODE]    get/set SPX|DPX|QPX|CPX compute partition
  drain IDX [--wait [--repartition MODE]]
                          stop scheduling onto a GPU (devices re-advertised
                          Unhealthy); --wait blocks until empty; --repartition
                          then flips the partition and undrains
  undrain IDX             return a drained GPU to service
  health [IDX [--run [--full] [--matrix] | --clear]]
                          list GPU self-test records; --run probes the GPU now
                          (same runner and policy as the agent); --clear puts
                          an unhealthy GPU back in service
  migrate --from BOLT_DB  import a reference agent's BoltDB state

(GC runs inside the agent daemon — event-driven + 60 s timer; there is no
offline GC because reclamation requires the live pod view.)
"""
from __future__ import annotations

import argparse
import json
import sys


def cmd_devices(args) -> int:
    if args.fake:
        from ..operator.fake import FakeBackend

        devices = FakeBackend().devices()
    else:
        from ..operator.amdsmi import AmdSmiBackend

        devices = AmdSmiBackend().devices()
    import dataclasses

    print(json.dumps([dataclasses.asdict(d) for d in devices], indent=2))
    return 0


def cmd_pods(args) -> int:
    from ..storage import Storage

    st = Storage(args.db)
    rows = []
    st.for_each(
        lambda pi: rows.append(
            {
                "pod": pi.key(),
                "containers": {
                    c: {"hash": d.hash, "resource": d.resource_name, "units": d.n_ids}
                    for c, d in pi.container_device_map.items()
                },
            }
        )
    )
    print(json.dumps(rows, indent=2))
    st.close()
    return 0


def cmd_masks(args) -> int:
    from ..isolation import AUX_MASK_PREFIX
    from ..storage import Storage

    st = Storage(args.db)
    out = {k[len(AUX_MASK_PREFIX):]: json.loads(v) for k, v in st.aux_items(AUX_MASK_PREFIX)}
    print(json.dumps(out, indent=2))
    st.close()
    return 0


def cmd_occupancy(args) -> int:
    from ..isolation import LimitsWriter
    from ..isolation.occupancy import report
    from ..storage import Storage

    st = Storage(args.db)
    limits = LimitsWriter(args.limits_dir)
    print(json.dumps(report(st, limits, state_dir=args.state_dir), indent=2))
    st.close()
    return 0


def cmd_partition(args) -> int:
    from elastic_gpu_agent_amd.operator import partition

    if args.mode:
        route = partition.set_mode(args.index, args.mode)
        print(f"gpu {args.index} partition set to {args.mode} via {route} "
              "(agent re-advertises on its next enumeration refresh)")
    print(json.dumps({"gpu": args.index,
                      "partition": partition.get(args.index)}))
    return 0


def cmd_drain(args) -> int:
    from ..drain import (clear_drain, list_drains, live_allocations_on, set_drain,
                         wait_drained)
    from ..isolation import LimitsWriter
    from ..storage import Storage

    st = Storage(args.db)
    try:
        if args.list:
            print(json.dumps(list_drains(st), indent=2))
            return 0
        if args.index is None:
            print("drain: an index is required (or --list)", file=sys.stderr)
            return 2
        limits = LimitsWriter(args.limits_dir)
        set_drain(st, args.index, mode=args.repartition)
        remaining = live_allocations_on(st, args.index, limits)
        print(f"gpu {args.index} drained for scheduling "
              f"({len(remaining)} live allocation(s) remaining)")
        if not args.wait:
            for row in remaining:
                print(f"  waiting on {row['pod']}/{row['container']} ({row['resource']})")
            if args.repartition:
                print(f"re-run with --wait to repartition to {args.repartition} "
                      "once the GPU is empty")
            return 0
        ok = wait_drained(
            st, args.index, limits, timeout=args.timeout,
            progress=lambda rows: print(f"  {len(rows)} allocation(s) still live..."),
        )
        if not ok:
            print(f"timeout after {args.timeout}s; drain flag left set", file=sys.stderr)
            return 1
        print(f"gpu {args.index} is empty")
        if args.repartition:
            from elastic_gpu_agent_amd.operator import partition

            partition.set_mode(args.index, args.repartition)
            clear_drain(st, args.index)
            print(f"gpu {args.index} repartitioned to {args.repartition} and "
                  "returned to service (agent re-advertises on its next refresh)")
        return 0
    finally:
        st.close()


def cmd_undrain(args) -> int:
    from ..drain import clear_drain
    from ..storage import Storage

    st = Storage(args.db)
    clear_drain(st, args.index)
    st.close()
    print(f"gpu {args.index} returned to service "
          "(agent re-advertises on its next refresh)")
    return 0


def cmd_health(args) -> int:
    from ..isolation import health
    from ..storage import Storage

    st = Storage(args.db)
    try:
        if args.index is None:
            if args.run or args.clear:
                print("health: --run and --clear need a GPU index", file=sys.stderr)
                return 2
            print(json.dumps(health.list_health(st), indent=2))
            return 0
        if args.clear:
            health.clear_health(st, args.index)
            print(f"gpu {args.index} self-test record cleared "
                  "(agent re-advertises on its next refresh)")
            return 0
        if args.run:
            # same runner and same policy as the agent's monitor; an operator's
            # explicit run also probes a GPU that is already unhealthy, but a
            # pass does not heal it (only --clear does)
            kw = {"matrix": True} if args.matrix else {}
            result = health.subprocess_runner(args.index, args.timeout, full=args.full, **kw)
            rec = health.apply_result(st, args.index, result)
            print(json.dumps({k: v for k, v in rec.items() if k != "became_unhealthy"},
                             indent=2))
            return 0 if rec["passed"] else 1
        rec = health.get_health(st, args.index)
        print(json.dumps({str(args.index): rec} if rec else {}, indent=2))
        return 0
    finally:
        st.close()


def cmd_migrate(args) -> int:
    from ..storage import Storage, migrate_from_bolt

    st = Storage(args.db)
    n = migrate_from_bolt(getattr(args, "from"), st)
    print(f"migrated {n} pod records")
    st.close()
    return 0


def cmd_export_bolt(args) -> int:
    from ..storage import Storage
    from ..storage.boltcompat import export_storage_to_bolt

    st = Storage(args.db)
    n = export_storage_to_bolt(st, args.to)
    print(f"exported {n} pod records to BoltDB file {args.to} "
          "(readable by the reference agent)")
    st.close()
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="egpuctl")
    p.add_argument("--db", default="/host/var/lib/egpu/meta.db")
    p.add_argument("--limits-dir", default="/host/var/lib/egpu/limits")
    p.add_argument("--state-dir", default="/host/var/lib/egpu")
    sub = p.add_subparsers(dest="cmd", required=True)

    d = sub.add_parser("devices")
    d.add_argument("--fake", action="store_true")
    d.set_defaults(fn=cmd_devices)
    sub.add_parser("pods").set_defaults(fn=cmd_pods)
    sub.add_parser("masks").set_defaults(fn=cmd_masks)
    sub.add_parser("occupancy").set_defaults(fn=cmd_occupancy)
    m = sub.add_parser("migrate", help="import a reference BoltDB state file")
    m.add_argument("--from", required=True)
    m.set_defaults(fn=cmd_migrate)
    eb = sub.add_parser("export-bolt",
                        help="write the allocation state as a BoltDB file "
                             "(rollback to the reference agent)")
    eb.add_argument("--to", required=True)
    eb.set_defaults(fn=cmd_export_bolt)
    dr = sub.add_parser(
        "drain",
        help="stop scheduling onto a GPU; optionally wait-empty and repartition",
    )
    dr.add_argument("index", type=int, nargs="?", default=None)
    dr.add_argument("--list", action="store_true", help="show active drains")
    dr.add_argument("--wait", action="store_true",
                    help="block until no live allocation references the GPU")
    dr.add_argument("--timeout", type=float, default=600.0)
    dr.add_argument("--repartition", default=None,
                    choices=["SPX", "DPX", "QPX", "CPX"],
                    help="with --wait: set this partition once empty, then undrain")
    dr.set_defaults(fn=cmd_drain)
    ud = sub.add_parser("undrain", help="return a drained GPU to service")
    ud.add_argument("index", type=int)
    ud.set_defaults(fn=cmd_undrain)
    he = sub.add_parser(
        "health",
        help="list GPU self-test records; probe a GPU now; clear a record",
    )
    he.add_argument("index", type=int, nargs="?", default=None)
    he.add_argument("--run", action="store_true",
                    help="probe the GPU now and record the result; exits "
                         "non-zero when the probe fails")
    he.add_argument("--full", action="store_true",
                    help="with --run: whole-LDS, 1 GiB probe for a drained or idle GPU")
    he.add_argument("--matrix", action="store_true",
                    help="with --run: also run the matrix sweep (fp8, fp6, fp4, int8, "
                         "f16 and 16x16 MFMA paths)")
    he.add_argument("--clear", action="store_true",
                    help="forget the record: the GPU is advertised Healthy and probed again")
    he.add_argument("--timeout", type=float, default=60.0,
                    help="with --run: time limit of the probe")
    he.set_defaults(fn=cmd_health)
    pt = sub.add_parser("partition", help="get/set SPX|DPX|QPX|CPX compute partition")
    pt.add_argument("index", type=int)
    pt.add_argument("mode", nargs="?", default=None,
                    choices=[None, "SPX", "DPX", "QPX", "CPX"])
    pt.set_defaults(fn=cmd_partition)

    args = p.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
