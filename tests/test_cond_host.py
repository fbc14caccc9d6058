"""Host-side contract of the class-conditional architecture and the classifier-free samplers: the parameter table of a
DMME_ARCH_DDPM_COND plan, what plan creation refuses, the new symbols and constants, the chain tables, checkpoint compatibility."""

import ctypes as C

import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.models.ddpm import _Plan, _cfg_struct

DEFAULT = dict(in_channels=3, pos_dim=128, emb_dim=512, num_groups=32, dropout=0.1, channels_per_depth=(128, 256, 256, 256), num_blocks=2,
               attention_depths=(2,))
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)


def _host_plan(arch, num_classes=0, dtype=_lib.F32, B=2, num_heads=1):
    return _Plan(_cfg_struct(arch=arch, num_heads=num_heads, num_classes=num_classes, **DEFAULT), B, 32, 32, dtype, -1)


def _numel(plan):
    return int(plan.lib.dmme_unet_plan_ref_numel(plan.h))


def test_conditional_plan_appends_one_entry():
    base, cond = _host_plan(_lib.ARCH_DDPM), _host_plan(_lib.ARCH_DDPM_COND, 10)
    tb, tc = base.param_table(), cond.param_table()
    assert len(tb) == 305 and len(tc) == 306
    assert tc[:305] == tb  # name, shape, offset, is_buffer
    assert tc[305] == ("label_emb.weight", (11, 512), _numel(base), False)
    assert _numel(cond) == _numel(base) + 11 * 512
    # everything DDPM-like is the DDPM plan's: op labels apart from the label op, gradient buckets apart from the longer last one
    lib = base.lib

    def labels(p):
        buf, f, b = C.create_string_buffer(160), C.c_double(), C.c_double()
        out = []
        for i in range(lib.dmme_unet_plan_num_ops(p.h)):
            _lib.check(lib.dmme_unet_plan_op_info(p.h, i, buf, 160, C.byref(f), C.byref(b)))
            out.append(buf.value.decode())
        return out

    lb, lc = labels(base), labels(cond)
    assert lc.count("label_cond_kernel") == 1 and [v for v in lc if v != "label_cond_kernel"] == lb

    def buckets(p):
        off, num, bk = (C.c_int64 * 64)(), (C.c_int64 * 64)(), (C.c_int * 64)()
        n = lib.dmme_unet_plan_grad_buckets(p.h, off, num, bk, 64)
        return [(off[i], num[i], bk[i]) for i in range(n)]

    bb, bc = buckets(base), buckets(cond)
    last = max(b for _, _, b in bc)
    assert sum(n for _, n, _ in bc) == _numel(cond)
    assert last == max(b for _, _, b in bb) and last >= 3
    assert sorted(bc) == sorted(bb + [(tc[305][2], 11 * 512, last)])  # the DDPM plan's buckets; the table rides in the last, with the time MLP


@pytest.mark.parametrize("dtype", [_lib.BF16X3, _lib.F16R32])
def test_conditional_plan_refuses_the_split_precisions(dtype):
    with pytest.raises(NotImplementedError):  # DMME_ERR_UNSUPPORTED
        _host_plan(_lib.ARCH_DDPM_COND, 10, dtype)


def test_conditional_plan_refuses_zero_classes():
    with pytest.raises(ValueError):  # DMME_ERR_INVALID
        _host_plan(_lib.ARCH_DDPM_COND, 0)


@pytest.mark.parametrize("arch,heads", [(_lib.ARCH_DDPM, 1), (_lib.ARCH_IDDPM, 4)])
def test_num_classes_is_ignored_by_the_existing_architectures(arch, heads):
    a, b = _host_plan(arch, 0, num_heads=heads), _host_plan(arch, 10, num_heads=heads)
    assert a.param_table() == b.param_table() and _numel(a) == _numel(b)
    assert int(a.lib.dmme_unet_plan_workspace_bytes(a.h)) == int(b.lib.dmme_unet_plan_workspace_bytes(b.h))
    assert a.lib.dmme_unet_plan_num_ops(a.h) == b.lib.dmme_unet_plan_num_ops(b.h)


def test_new_symbols_and_constants():
    lib = _lib.lib()
    assert lib.dmme_version() >= 110
    for name in ("dmme_unet_forward_cond", "dmme_unet_backward_cond", "dmme_unet_backward_input_cond", "dmme_label_dropout", "dmme_cfg_step",
                 "dmme_chain_update_cfg", "dmme_cfg_chain_step"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert (_lib.CHAIN_DDPM_CFG, _lib.CHAIN_GDDIM_CFG, _lib.ARCH_DDPM_COND) == (6, 7, 3)
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.CSRC), "..", "include", "dmme_hip.h")).read()
    assert "DMME_CHAIN_DDPM_CFG = 6" in header and "DMME_CHAIN_GDDIM_CFG = 7" in header and "DMME_ARCH_DDPM_COND = 3" in header


def test_label_less_entry_points_refuse_a_conditional_host_plan():
    """the refusal precedes any launch, so a host plan shows it: a label-less call never runs with garbage labels"""
    plan = _host_plan(_lib.ARCH_DDPM_COND, 10)
    lib, one = plan.lib, C.c_void_p(64)
    for rc in (lib.dmme_unet_forward(plan.h, one, one, one, 1, one, one, None, None),
               lib.dmme_unet_forward_nograd(plan.h, one, one, one, 1, one, one, None, None),
               lib.dmme_chain_step(plan.h, one, one, one, one, _lib.CHAIN_DDPM, one, one, one, None),
               lib.dmme_unet_backward(plan.h, one, one, one, one, 2, one, one, one, None, one, None, None),
               lib.dmme_unet_backward_input(plan.h, one, one, one, one, 2, one, one, one, None, one, None)):
        assert rc == -1 and (b"_cond" in lib.dmme_last_error() or b"cfg_chain_step" in lib.dmme_last_error())
    base = _host_plan(_lib.ARCH_DDPM)
    assert lib.dmme_unet_forward_cond(base.h, one, one, one, 1, one, one, one, None, 0, None, None) == -1


def test_chain_tables_carry_the_scale_in_column_3():
    net = dmme_amd.ConditionalUNet(num_classes=3, **TINY_KW)
    for proc, base in ((dmme_amd.ClassifierFreeDDPM(net, 8, guidance_scale=2.5), dmme_amd.DDPM(net, 8)),
                       (dmme_amd.ClassifierFreeDDIM(net, 8, 4, eta=0.5, guidance_scale=2.5), dmme_amd.GeneralizedDDIM(net, 8, 4, eta=0.5))):
        (n, rows, ttab), (nb, rb, tb) = proc._chain_tables(), base._chain_tables()
        assert (n, ttab) == (nb, tb) and len(rows) == len(rb)
        assert all(r[:3] == b[:3] and b[3] == 0.0 and r[3] == 2.5 for r, b in zip(rows, rb))
    assert dmme_amd.ClassifierFreeDDPM(net, 8)._chain_kind == 6 and dmme_amd.ClassifierFreeDDIM(net, 8, 4)._chain_kind == 7
    with pytest.raises(TypeError):
        dmme_amd.ClassifierFreeDDPM(dmme_amd.UNet(**TINY_KW), 8)


def test_unconditional_checkpoint_is_a_prefix():
    unet = dmme_amd.UNet(**TINY_KW)
    cond = dmme_amd.ConditionalUNet(num_classes=3, **TINY_KW)
    assert cond.null_label == 3 and tuple(cond.label_emb.weight.shape) == (4, 8)
    res = cond.load_state_dict(unet.state_dict(), strict=False)
    assert res.missing_keys == ["label_emb.weight"] and not res.unexpected_keys
    n = unet.flat_parameters().numel()
    assert torch.equal(cond.flat_parameters()[:n], unet.flat_parameters())
    assert list(cond.state_dict())[-1] == "label_emb.weight"


def test_host_side_label_check():
    from dmme_amd.models.cond import class_labels

    assert class_labels([0, 3], 2, 3, "cpu").tolist() == [0, 3]  # the null label is a label
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError):
            class_labels(bad, 2, 3, "cpu")
    with pytest.raises(ValueError):
        class_labels([0], 2, 3, "cpu")
