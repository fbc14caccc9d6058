"""CPU: the C-ABI library loads and exports every symbol include/dmme_hip.h declares; the
ctypes prototypes list exactly that set; host-only entry points behave (no GPU compute)."""

import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "dmme_hip.h")).read()
    return sorted(set(re.findall(r"DMME_API[^;(]*?\b(dmme_\w+)\s*\(", text)))


def test_header_declares_entry_points():
    names = declared_symbols()
    assert len(names) >= 30
    for must in ("dmme_unet_plan_create", "dmme_unet_forward", "dmme_q_sample", "dmme_ddpm_step", "dmme_ddim_step", "dmme_conv2d"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from dmme_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    h = C.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(h, name), f"{name} declared in include/dmme_hip.h but not exported"
    assert sorted(_lib.PROTOTYPES) == declared_symbols()
    assert _lib.lib().dmme_version() >= 100


def test_plan_is_host_only_and_reports_errors():
    from dmme_amd import _lib

    lib = _lib.lib()
    cfg = _lib.UNetCfg()
    cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout = 3, 128, 512, 32, 0.1
    cfg.num_depths, cfg.num_blocks, cfg.num_attention_depths = 4, 2, 1
    for i, c in enumerate((128, 256, 256, 256)):
        cfg.channels_per_depth[i] = c
    cfg.attention_depths[0] = 2
    h = C.c_void_p()
    assert lib.dmme_unet_plan_create(C.byref(cfg), 128, 32, 32, _lib.BF16, -1, C.byref(h)) == 0
    assert lib.dmme_unet_plan_num_params(h) == 305
    assert lib.dmme_unet_plan_ref_numel(h) == 32_416_643 + 64  # parameters + the sinusoid buffer
    assert lib.dmme_unet_plan_workspace_bytes(h) > 0 and lib.dmme_unet_plan_packed_bytes(h) > 2 * 32_416_643
    assert lib.dmme_unet_plan_dropmask_numel(h) == 128 * 4736
    n_ops = lib.dmme_unet_plan_num_ops(h)
    # launches = ops minus the GroupNorms finished by their producing convs' epilogues (8x8 / 4x4 / 16x16 whole-image tiles) or by
    # their consuming conv's parameter fill (the norms in front of the persistent 3x3 / the activation-stationary 1x1 kernel)
    n_launch = lib.dmme_unet_plan_num_launches(h)
    # ... and, since round 3, minus the layers of the 8x8 / 4x4 maps: three level-engine launches stand for 57 convs, norms and the
    # middle attention (csrc/lvl_engine.hip)
    buf = C.create_string_buffer(1024)
    assert lib.dmme_unet_plan_level_info(h, buf, 1024) == 0
    info = buf.value.decode()
    assert info.startswith("runs=3") and info.count("map=8x8") == 2 and info.count("map=4x4") == 1 and info.count("workgroups=256") == 3, info
    # ... and, since round 4, minus the seven 1x1 residual convs of the 32x32 / 16x16 levels that run inside their block's conv2 (51 now)
    # ... and, since round 5, minus the proj convs of the five 16x16 attention blocks, which run inside the attention launch (45 now)
    assert n_ops >= n_launch >= 43 and n_launch <= 50, (n_ops, n_launch)
    label = C.create_string_buffer(128)
    fl, by = C.c_double(), C.c_double()
    total = 0.0
    for i in range(n_ops):
        assert lib.dmme_unet_plan_op_info(h, i, label, 128, C.byref(fl), C.byref(by)) == 0
        total += fl.value
    # algorithmic FLOPs of one batch-128 forward: 128 x 9.809 GFLOP, time-MLP counted once
    assert abs(total / 128 / 9.809e9 - 1) < 0.01
    lib.dmme_unet_plan_destroy(h)
    # invalid arguments come back as a status + message, never an exception / crash
    cfg.num_groups = 7
    assert lib.dmme_unet_plan_create(C.byref(cfg), 1, 32, 32, _lib.F32, -1, C.byref(h)) == -1
    assert b"num_groups" in lib.dmme_last_error()
    with pytest.raises(ValueError):
        _lib.check(-1, "x")
    with pytest.raises(NotImplementedError):
        _lib.check(-2, "x")


def _default_cfg():
    from dmme_amd import _lib

    cfg = _lib.UNetCfg()
    cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout = 3, 128, 512, 32, 0.1
    cfg.num_depths, cfg.num_blocks, cfg.num_attention_depths = 4, 2, 1
    for i, c in enumerate((128, 256, 256, 256)):
        cfg.channels_per_depth[i] = c
    cfg.attention_depths[0] = 2
    return cfg


def _plan_labels(batch, dtype, route=None):
    from dmme_amd import _lib

    lib = _lib.lib()
    old = os.environ.get("DMME_DEBUG_ROUTE")
    if route is not None:
        os.environ["DMME_DEBUG_ROUTE"] = route
    try:
        h = C.c_void_p()
        cfg = _default_cfg()
        assert lib.dmme_unet_plan_create(C.byref(cfg), batch, 32, 32, dtype, -1, C.byref(h)) == 0
    finally:
        if route is not None:
            if old is None:
                os.environ.pop("DMME_DEBUG_ROUTE", None)
            else:
                os.environ["DMME_DEBUG_ROUTE"] = old
    label = C.create_string_buffer(128)
    fl, by = C.c_double(), C.c_double()
    out, total = [], 0.0
    for i in range(lib.dmme_unet_plan_num_ops(h)):
        assert lib.dmme_unet_plan_op_info(h, i, label, 128, C.byref(fl), C.byref(by)) == 0
        out.append(label.value.decode())
        total += fl.value
    n = lib.dmme_unet_plan_num_launches(h)
    lib.dmme_unet_plan_destroy(h)
    return out, n, total


def test_plan_fuses_residual_convs_into_conv2_where_the_persistent_kernel_runs_it():
    """host logic of assign_rseg (csrc/plan.hip), no GPU: at the benchmark batch the seven channel-changing ResBlocks of the 32x32 /
    16x16 levels lose their 1x1 launch (five on the 256-pixel tiles, two on the 128-pixel ones), at batch 32 the three whose conv2 the
    persistent kernel takes, at batch 1 none; never in fp32 / fp16r32 plans; the switch restores the launches; FLOPs are conserved."""
    from dmme_amd import _lib

    fused = lambda labels: sum(1 for l in labels if l.startswith("(residual 1x1 conv"))
    l128, n128, f128 = _plan_labels(128, _lib.BF16)
    l128_off, n128_off, f128_off = _plan_labels(128, _lib.BF16, "no_rseg")
    assert fused(l128) == 7 and fused(l128_off) == 0 and n128_off == n128 + 7
    assert sum(1 for l in l128 if l == "conv3x3_ws2_kernel<11,res>") == 5 and sum(1 for l in l128 if l == "conv3x3_ws2_kernel<7,128,res>") == 2
    assert abs(f128 / f128_off - 1) < 1e-12
    assert fused(_plan_labels(128, _lib.F16)[0]) == 7
    assert fused(_plan_labels(32, _lib.BF16)[0]) == 3
    assert fused(_plan_labels(1, _lib.BF16)[0]) == 0
    for dt in (_lib.F32, _lib.F16R32):
        assert fused(_plan_labels(128, dt)[0]) == 0


def _host_plan_backward(batch, dtype, env=None, arch=None):
    """(bucket table [(offset, numel, bucket)], ref_numel, bwd_summary) of a host-only plan of the default UNet"""
    from dmme_amd import _lib

    lib = _lib.lib()
    cfg = _default_cfg()
    if arch is not None:
        cfg.arch, cfg.num_classes = arch, 10
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        h = C.c_void_p()
        assert lib.dmme_unet_plan_create(C.byref(cfg), batch, 32, 32, dtype, -1, C.byref(h)) == 0
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    off, num, bucket = (C.c_int64 * 64)(), (C.c_int64 * 64)(), (C.c_int * 64)()
    n = lib.dmme_unet_plan_grad_buckets(h, off, num, bucket, 64)
    assert 1 <= n <= 64
    buf = C.create_string_buffer(4096)
    assert lib.dmme_unet_plan_bwd_summary(h, buf, 4096) == 0
    ref_numel = lib.dmme_unet_plan_ref_numel(h)
    lib.dmme_unet_plan_destroy(h)
    return [(off[i], num[i], bucket[i]) for i in range(n)], ref_numel, buf.value.decode()


DEFAULT_BUCKETS = [(23908288, 5616000, 0), (32412992, 3715, 0), (19249856, 4658432, 1), (12557248, 6692608, 2), (10523072, 2034176, 3),
                   (29524288, 2888704, 3), (4682944, 5840128, 4), (0, 4682944, 5)]


def test_host_plan_cuts_the_default_unet_into_six_gradient_buckets():
    """host logic of plan_grad_buckets (csrc/plan_bwd.hip), no GPU: a plan without a device announces the bucket table a device plan
    hands over (tests/test_gpu_train.py asserts the same three balance conditions on the GPU) - 8 ranges in 6 buckets that tile the
    flat gradient, whatever the batch and dtype."""
    from dmme_amd import _lib

    for batch, dtype in ((128, _lib.BF16), (32, _lib.F16), (1, _lib.BF16), (2, _lib.F32), (128, _lib.F16R32)):
        table, n, _ = _host_plan_backward(batch, dtype)
        assert table == DEFAULT_BUCKETS, (batch, dtype, table)
        pos = 0
        for o, m, _b in sorted(table):
            assert o == pos, (o, pos)
            pos = o + m
        assert pos == n
        nb = max(b for _, _, b in table) + 1
        per_bucket = [sum(m for _, m, b in table if b == k) for k in range(nb)]
        assert nb == 6 and [b for _, _, b in table] == sorted(b for _, _, b in table)
        assert nb >= 4 and max(per_bucket) <= 0.26 * n and per_bucket[-1] <= 0.15 * n, per_bucket


def test_host_plan_reports_the_deferred_backward_tables():
    """host logic of build_wgrad_group / plan_deferred_reductions (csrc/plan_bwd.hip), no GPU: the grouped weight-gradient, column-sum
    and bias tables of the benchmark plan; an fp32 plan has no grouped weight gradient and the column sums of every conv."""
    from dmme_amd import _lib

    _, _, s = _host_plan_backward(128, _lib.BF16)
    assert s.startswith("wgrad_group3x3_layers=47 wgrad_group3x3_jobs=3840 wgrad_group1x1_layers=25 wgrad_group1x1_jobs=912 "
                        "colsum_group_jobs=160 bias_group_jobs=1424"), s
    _, _, s = _host_plan_backward(2, _lib.F32)
    assert s.startswith("wgrad_group3x3_layers=0 wgrad_group3x3_jobs=0 wgrad_group1x1_layers=0 wgrad_group1x1_jobs=0 colsum_group_jobs=285 "), s


def test_host_plan_without_buckets_is_one_piece():
    """the one-piece answer include/dmme_hip.h documents: the classifier, DMME_NO_GRAD_BUCKETS; grad_buckets=3 cuts three"""
    from dmme_amd import _lib

    for kw in (dict(arch=_lib.ARCH_CLASSIFIER), dict(env={"DMME_NO_GRAD_BUCKETS": "1"})):
        table, n, _ = _host_plan_backward(128, _lib.BF16, **kw)
        assert table == [(0, n, 0)], (kw, table)
    table, n, _ = _host_plan_backward(128, _lib.BF16, env={"DMME_DEBUG_ROUTE": "grad_buckets=3"})
    assert len(table) == 5 and max(b for _, _, b in table) + 1 == 3 and sum(m for _, m, _b in table) == n, table
