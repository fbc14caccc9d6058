#!/usr/bin/env python
"""Which kernels every plan of a matrix of networks / batches / precisions / route switches launches, from host-only plans
(device = -1: no GPU is touched).  Per plan: the creation status, the ordered op labels (one SHA-256), the launch count, the workspace
bytes, the backward summary (one SHA-256 over its sorted key=value pairs: the library lists the dgrad[...] pairs in hash-map order), the
backward workspace bytes and the bytes of the backward's packed weights.

  python tools/plan_routes.py               rewrite tests/plan_routes.json from the library the package loads
  python tools/plan_routes.py --check       compare that library against tests/plan_routes.json (what tests/test_plan_routes.py does)
  python tools/plan_routes.py --dump KEY    one plan's full listing (diff two builds by eye: DMME_LIB_PATH selects the library)
  python tools/plan_routes.py --keys        the keys of the matrix

A routing refactor must leave tests/plan_routes.json as the build before it wrote it."""

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "plan_routes.json")

BATCHES = (1, 2, 8, 32, 128)
PRECISIONS = ("fp32", "bf16", "fp16", "fp16r32", "bf16x3")
# name -> (constructor arguments of models.ddpm._cfg_struct, image side)
DEFAULT = dict(in_channels=3, pos_dim=128, emb_dim=512, num_groups=32, dropout=0.1, channels_per_depth=(128, 256, 256, 256), num_blocks=2, attention_depths=(2,))
NETWORKS = {
    "ddpm": (DEFAULT, 32),
    "iddpm": (dict(DEFAULT, dropout=0.3, attention_depths=(2, 3), arch=1, num_heads=4), 32),
    "iddpm64": (dict(DEFAULT, dropout=0.3, attention_depths=(3, 4), arch=1, num_heads=4), 64),  # bench.py --model iddpm64
    "classifier": (dict(DEFAULT, dropout=0.0, arch=2, num_classes=10), 32),                     # guidance.EncoderClassifier()
    "tiny": (dict(DEFAULT, pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3), 32),  # oracle.unet.TINY
}


def switch_rows():
    """(id, environment) of every forward switch row of tests/test_gpu_switches.py"""
    from tests.test_gpu_switches import FORWARD

    return [("+".join(f"{k}={v}" if v != "1" else k for k, v in env.items()), env) for env, _ in FORWARD]


def backward_switch_rows():
    """(id, environment) of every backward switch of tests/test_gpu_switches.py, each set alone"""
    from tests.test_gpu_switches import BACKWARD

    return [(name, {name: "1"}) for name in BACKWARD]


def matrix():
    """[(key, network, batch, precision, environment)]"""
    out = []
    for net in NETWORKS:
        for B in BATCHES:
            for prec in PRECISIONS:
                out.append((f"{net}/b{B}/{prec}", net, B, prec, {}))
    for net in ("ddpm", "iddpm", "iddpm64", "classifier"):
        for B in (BATCHES if net == "ddpm" else (1, 128)):
            for sid, env in switch_rows():
                out.append((f"{net}/b{B}/bf16/{sid}", net, B, "bf16", env))
    have = {key for key, *_ in out}  # (a few switches are in both lists)
    for net in ("ddpm", "iddpm", "classifier"):
        for B in (32, 128):
            for sid, env in backward_switch_rows():
                if f"{net}/b{B}/bf16/{sid}" not in have:
                    out.append((f"{net}/b{B}/bf16/{sid}", net, B, "bf16", env))
    return out


def listing(net, B, prec, env):
    """status, op labels, launches, workspace bytes, backward summary, backward workspace and packed bytes of one host-only plan"""
    from dmme_amd import _lib
    from dmme_amd.models.ddpm import _cfg_struct
    from tests.gpu_util import route_env

    lib = _lib.lib()
    kw, side = NETWORKS[net]
    cfg = _cfg_struct(**kw)
    h = C.c_void_p()
    with route_env(env):  # (the labels and the summary are answered under the plan's switches as well: a launch would read them again)
        rc = lib.dmme_unet_plan_create(C.byref(cfg), B, side, side, _lib.dtype_code(prec), -1, C.byref(h))
        if rc != 0:
            return {"status": rc}
        label, fl, by = C.create_string_buffer(128), C.c_double(), C.c_double()
        labels = []
        for i in range(lib.dmme_unet_plan_num_ops(h)):
            _lib.check(lib.dmme_unet_plan_op_info(h, i, label, 128, C.byref(fl), C.byref(by)), "op_info")
            labels.append(label.value.decode())
        buf = C.create_string_buffer(16384)
        _lib.check(lib.dmme_unet_plan_bwd_summary(h, buf, 16384), "bwd_summary")
        out = {"status": 0, "labels": labels, "launches": lib.dmme_unet_plan_num_launches(h), "workspace_bytes": lib.dmme_unet_plan_workspace_bytes(h),
               "bwd_summary": sorted(buf.value.decode().split()), "bwd_workspace_bytes": lib.dmme_unet_plan_bwd_workspace_bytes(h),
               "packed_bwd_bytes": lib.dmme_unet_plan_packed_bwd_bytes(h)}
        lib.dmme_unet_plan_destroy(h)
    return out


def entry(full):
    if full["status"] != 0:
        return {"status": full["status"]}
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()
    return {"status": 0, "labels_sha256": sha(full["labels"]), "launches": full["launches"], "workspace_bytes": full["workspace_bytes"],
            "bwd_summary_sha256": sha(full["bwd_summary"]), "bwd_workspace_bytes": full["bwd_workspace_bytes"], "packed_bwd_bytes": full["packed_bwd_bytes"]}


def table():
    return {key: entry(listing(net, B, prec, env)) for key, net, B, prec, env in matrix()}


def mismatches(got, want):
    """keys whose entries differ (or exist on one side only)"""
    return [k for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--dump", metavar="KEY")
    ap.add_argument("--keys", action="store_true")
    args = ap.parse_args()
    if args.keys:
        print("\n".join(k for k, *_ in matrix()))
        return 0
    if args.dump:
        rows = [m for m in matrix() if m[0] == args.dump]
        if not rows:
            print(f"no such key: {args.dump} (--keys lists them)", file=sys.stderr)
            return 2
        full = listing(*rows[0][1:])
        print(f"{args.dump}: status {full['status']}")
        if full["status"] == 0:
            print(f"launches {full['launches']}  workspace_bytes {full['workspace_bytes']}  bwd_workspace_bytes {full['bwd_workspace_bytes']}  packed_bwd_bytes {full['packed_bwd_bytes']}")
            for i, l in enumerate(full["labels"]):
                print(f"{i:4d}  {l}")
            print("\n".join(full["bwd_summary"]))
        return 0
    got = table()
    if args.check:
        with open(TABLE) as f:
            bad = mismatches(got, json.load(f))
        print("\n".join(f"differs: {k}" for k in bad) or f"{len(got)} plans: identical")
        return 1 if bad else 0
    with open(TABLE, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{TABLE}: {len(got)} plans")
    return 0


if __name__ == "__main__":
    sys.exit(main())
