"""CPU tests of the host logic that lets biased SoWLinear layers into the flat bucket: factor_parameters(biases=True),
FactorBucket.attach with bias members, and FactorAdamW with param groups (segment table, per-group steps, state dict).
No kernel is launched."""
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN


def _roberta(layers=2):
    transformers = pytest.importorskip("transformers")
    from sow_amd import SoWConfig, prepare_sow
    with open(os.path.join(GOLDEN, "prepare_names.json")) as f:
        targets = json.load(f)["roberta"]["targets"]
    cfg = transformers.RobertaConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=layers, num_attention_heads=12,
                                     vocab_size=50265, max_position_embeddings=514, type_vocab_size=1)
    model = transformers.AutoModelForCausalLM.from_config(cfg)
    return prepare_sow(model, SoWConfig(target_modules=targets, rank=8, init_method="normal", decompose=None, device="cpu"))


@pytest.fixture(scope="module")
def roberta():
    return _roberta(2)


def _net(bias=True, rank=4):
    from sow_amd import SoWLinear
    net = nn.Sequential()
    net.add_module("a", SoWLinear(12, 10, bias=bias, rank=rank, init_method="normal"))
    net.add_module("b", SoWLinear(10, 70, bias=bias, rank=rank, init_method="normal"))
    return net


def test_roberta_biased_layers_attach_and_biases_form_the_tail(roberta):
    from sow_amd import FactorBucket, SoWLinear, factor_parameters
    sow = [(n, m) for n, m in roberta.named_modules() if isinstance(m, SoWLinear)]
    assert len(sow) == 12 and all(m.bias is not None for _, m in sow)      # 6 per encoder layer, every one biased
    params = factor_parameters(roberta, biases=True)
    assert len(params) == 36
    assert [id(p) for p in params[24:]] == [id(m.bias) for _, m in sow]    # module order, after every A and B
    assert [id(p) for p in params[:24]] == [id(p) for p in factor_parameters(roberta)]
    bucket = FactorBucket(params)
    assert bucket.attach(roberta) == 12
    # one contiguous run at the end of the flat buffers, 64-element slots, .grad the view of flat_grad
    tail0 = bucket.offsets[24]
    assert all(o < tail0 for o in bucket.offsets[:24])
    off = tail0
    esz = bucket.flat_grad.element_size()
    for (_, m), o in zip(sow, bucket.offsets[24:]):
        assert o == off
        assert m.bias.data_ptr() == bucket.flat_param.data_ptr() + o * esz
        assert m.bias.grad.data_ptr() == bucket.flat_grad.data_ptr() + o * esz == bucket.grad_ptr(m.bias)
        assert m._grad_sink.pbias is m.bias
        off += (m.bias.numel() + 63) // 64 * 64
    assert off == bucket.padded_numel
    names = bucket.exclude_from_ddp(roberta)
    assert len(names) == 36
    bias_names = [n for n in names if n.endswith(".bias")]
    assert bias_names == [n + ".bias" for n, _ in sow] and len(bias_names) == 12
    # two encoder blocks of six layers each
    assert sorted(b["n"] for b in bucket._blocks.values()) == [6, 6]


def test_bucket_without_biases_behaves_as_before(roberta):
    from sow_amd import FactorBucket, SoWLinear, factor_parameters
    from sow_amd.optimizer import FactorAdamW
    model = _roberta(1)
    bucket = FactorBucket(factor_parameters(model))
    assert len(bucket.params) == 12
    assert bucket.attach(model) == 0                          # every RoBERTa layer is biased: all keep autograd
    assert not any(hasattr(m, "_grad_sink") for m in model.modules())
    net = _net(bias=False)
    net.add_module("c", SoWLinear(70, 6, bias=True, rank=4, init_method="normal"))
    b2 = FactorBucket(factor_parameters(net))
    assert b2.attach(net) == 2 and net.a._grad_sink.pbias is None and not hasattr(net.c, "_grad_sink")
    assert [n for n in b2.exclude_from_ddp(net) if n.endswith("bias")] == []
    opt = FactorAdamW(b2)
    assert sorted(opt.state_dict()) == ["betas", "eps", "exp_avg", "exp_avg_sq", "lr", "numel", "step", "weight_decay"]
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["params"] is b2.params
    with pytest.raises(RuntimeError):
        opt.segments()


def test_biased_rank_64_layer_is_not_attached():
    from sow_amd import FactorBucket, SoWLinear, factor_parameters
    from sow_amd.dp import bias_route_ok
    net = nn.Sequential()
    for name, r in (("r63", 63), ("r64", 64), ("r72", 72), ("r73", 73), ("r256", 256), ("r258", 258)):
        net.add_module(name, SoWLinear(300, 280, bias=True, rank=r, init_method="normal"))
    net.add_module("r64nb", SoWLinear(300, 280, bias=False, rank=64, init_method="normal"))
    bucket = FactorBucket(factor_parameters(net, biases=True))
    assert bucket.attach(net) == 4
    attached = {n for n, m in net.named_children() if hasattr(m, "_grad_sink")}
    assert attached == {"r63", "r72", "r256", "r64nb"}
    # the rank-64 layer keeps autograd, and AccumulateGrad adds into the same flat views
    assert net.r64.bias.grad.data_ptr() == bucket.grad_ptr(net.r64.bias)
    assert [bias_route_ok(r) for r in (1, 63, 64, 65, 66, 256, 257, 258)] == [True, True, False, False, True, True, False, False]
    # a sink refuses a call whose bias is not the one it was attached with
    s = net.r63._grad_sink
    A, B = net.r63.downscale_weights[0], net.r63.upscale_weights[0]
    assert s.usable(A, B, net.r63.bias) and not s.usable(A, B, None) and not s.usable(A, B, net.r72.bias)
    s0 = net.r64nb._grad_sink
    A0, B0 = net.r64nb.downscale_weights[0], net.r64nb.upscale_weights[0]
    assert s0.usable(A0, B0) and s0.usable(A0, B0, None) and not s0.usable(A0, B0, net.r63.bias)


def _two_group_opt(**kw):
    from sow_amd import FactorBucket, factor_parameters
    from sow_amd.optimizer import FactorAdamW
    net = _net()
    params = factor_parameters(net, biases=True)
    bucket = FactorBucket(params)
    groups = [{"params": params[:4], "lr": 1e-2, "weight_decay": 0.1}, {"params": params[4:], "lr": 3e-4, "weight_decay": 0.0}]
    return net, bucket, params, FactorAdamW(bucket, betas=(0.9, 0.95), eps=1e-6, param_groups=groups, **kw)


def test_param_groups_segment_table():
    net, bucket, params, opt = _two_group_opt()
    # slots: A_a 48 -> 64, B_a 40 -> 64, A_b 40 -> 64, B_b 280 -> 320, bias_a 10 -> 64, bias_b 70 -> 128
    assert bucket.offsets == [0, 64, 128, 192, 512, 576] and bucket.padded_numel == 704
    assert opt.segments() == [(0, 512, 1e-2, 0.1, 1), (512, 704, 3e-4, 0.0, 1)]
    assert opt.param_groups[0]["lr"] == 1e-2 and opt.param_groups[1]["weight_decay"] == 0.0
    assert opt.param_groups[0]["betas"] == (0.9, 0.95)
    opt.param_groups[1]["lr"] = 5e-4                  # a driver's scheduler writes per group
    opt.group_steps = [3, 9]
    assert opt.segments() == [(0, 512, 1e-2, 0.1, 4), (512, 704, 5e-4, 0.0, 10)]
    # interleaved groups: adjacent slots of one group merge, every slot keeps its padding
    from sow_amd.optimizer import FactorAdamW
    g = [{"params": [params[0], params[3], params[4]], "lr": 1.0, "weight_decay": 0.5},
         {"params": [params[1], params[2], params[5]], "lr": 2.0, "weight_decay": 0.0}]
    o2 = FactorAdamW(bucket, param_groups=g)
    assert o2.segments() == [(0, 64, 1.0, 0.5, 1), (64, 192, 2.0, 0.0, 1), (192, 576, 1.0, 0.5, 1), (576, 704, 2.0, 0.0, 1)]
    # defaults of the constructor fill a group that names neither
    o3 = FactorAdamW(bucket, lr=7e-3, weight_decay=0.25, param_groups=[{"params": params}])
    assert o3.segments() == [(0, 704, 7e-3, 0.25, 1)]


def test_param_groups_must_partition_the_bucket():
    from sow_amd.optimizer import FactorAdamW
    net, bucket, params, _ = _two_group_opt()
    with pytest.raises(ValueError, match="in no param group"):
        FactorAdamW(bucket, param_groups=[{"params": params[:5]}])
    with pytest.raises(ValueError, match="param groups 0 and 1"):
        FactorAdamW(bucket, param_groups=[{"params": params[:5]}, {"params": params[4:]}])
    with pytest.raises(ValueError, match="param groups 0 and 0"):
        FactorAdamW(bucket, param_groups=[{"params": params + params[:1]}])
    with pytest.raises(ValueError, match="not in the bucket"):
        FactorAdamW(bucket, param_groups=[{"params": params + [nn.Parameter(torch.zeros(3))]}])


def test_reset_state_of_one_group_keeps_the_other_groups_step(monkeypatch):
    from sow_amd import ops
    net, bucket, params, opt = _two_group_opt(state_dtype=torch.float32)
    for _ in range(3):                                # what three step() calls do to the counts (no kernel here)
        opt.group_steps = [s + 1 for s in opt.group_steps]
        opt.step_count += 1
    opt.exp_avg.fill_(1.0)
    opt.exp_avg_sq.fill_(2.0)
    calls = []

    def zero(tensors):                                # the one multi-tensor launch, on the CPU
        calls.append(len(tensors))
        for t in tensors:
            t.zero_()

    monkeypatch.setattr(ops, "zero_", zero)
    opt.reset_state(0)
    assert opt.group_steps == [0, 3] and opt.step_count == 3
    assert calls == [2]                               # ONE call: the group's range of exp_avg and of exp_avg_sq
    assert float(opt.exp_avg[:512].abs().sum()) == 0 and float(opt.exp_avg_sq[:512].abs().sum()) == 0
    assert bool((opt.exp_avg[512:] == 1.0).all()) and bool((opt.exp_avg_sq[512:] == 2.0).all())
    assert opt.segments() == [(0, 512, 1e-2, 0.1, 1), (512, 704, 3e-4, 0.0, 4)]
    with pytest.raises(ValueError):
        opt.reset_state(2)
    opt.reset_state()
    assert opt.group_steps == [0, 0] and opt.step_count == 0 and float(opt.exp_avg.abs().sum()) == 0


def test_param_group_state_dict_round_trips_and_parent_format_loads():
    from sow_amd.optimizer import FactorAdamW
    net, bucket, params, opt = _two_group_opt(state_dtype=torch.float32)
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    opt.group_steps, opt.step_count = [2, 11], 11
    opt.param_groups[0]["lr"] = 4e-3
    sd = opt.state_dict()
    parent_keys = {"betas", "eps", "exp_avg", "exp_avg_sq", "lr", "numel", "step", "weight_decay"}
    assert set(sd) == parent_keys | {"group_lr", "group_weight_decay", "group_steps"}
    assert sd["group_lr"] == [4e-3, 3e-4] and sd["group_weight_decay"] == [0.1, 0.0] and sd["group_steps"] == [2, 11]
    other = FactorAdamW(bucket, state_dtype=torch.float32, param_groups=[{"params": params[:4]}, {"params": params[4:]}])
    other.load_state_dict(sd)
    assert other.segments() == opt.segments() == [(0, 512, 4e-3, 0.1, 3), (512, 704, 3e-4, 0.0, 12)]
    assert other.betas == (0.9, 0.95) and other.eps == 1e-6 and other.step_count == 11
    assert torch.equal(other.exp_avg, opt.exp_avg) and torch.equal(other.exp_avg_sq, opt.exp_avg_sq)
    with pytest.raises(ValueError, match="number of param groups"):
        FactorAdamW(bucket, param_groups=[{"params": params}]).load_state_dict(sd)
    # a checkpoint written by the one-group optimizer (the format before param groups existed)
    old = FactorAdamW(bucket, lr=3e-3, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.2, state_dtype=torch.float32)
    old.exp_avg.normal_()
    old.step_count = 5
    parent = old.state_dict()
    assert set(parent) == parent_keys
    one = FactorAdamW(bucket, state_dtype=torch.float32, param_groups=[{"params": params}])
    one.load_state_dict(parent)
    assert one.segments() == [(0, 704, 3e-3, 0.2, 6)] and one.betas == (0.9, 0.98) and torch.equal(one.exp_avg, old.exp_avg)
    plain = FactorAdamW(bucket, state_dtype=torch.float32)
    plain.load_state_dict(parent)
    assert plain.step_count == 5 and plain.lr == 3e-3
