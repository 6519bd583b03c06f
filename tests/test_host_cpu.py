"""CPU tests of the host logic: C-ABI surface, module surgery, state-dict layout, checkpoint loader,
flat factor bucket + world_size-2 gloo all-reduce.  No GPU compute is attempted here."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN, ROOT, load_golden


def test_cabi_exports_every_declared_symbol():
    from sow_amd import _lib
    header = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(sow_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.sow_version() >= 100
    assert loaded.sow_error_string(-5) == b"workspace too small"
    assert loaded.sow_workspace_bytes(32768, 512, 512, 50, 0, 0, 1) > 0
    assert loaded.sow_h_save_elems(100, 50) == 6400 and loaded.sow_h_save_elems(100, 70) == 7000


def test_product_has_no_cpu_fallback_and_no_oracle_import():
    from sow_amd import SoWLinear, ops
    layer = SoWLinear(16, 12, rank=4, init_method="normal")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(torch.randn(2, 16))
    with pytest.raises(RuntimeError):
        layer.accumulate()
    with pytest.raises(RuntimeError):
        ops.qr_thin(torch.randn(8, 4), 2)
    with pytest.raises(RuntimeError):
        SoWLinear(16, 12, rank=4, init_method="normal_QR")  # reference hard-codes "cuda" there too
    for dirpath, _, files in os.walk(os.path.join(ROOT, "sow_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_sowlinear_surface_matches_reference():
    from sow_amd import SoWLinear, SoWParameter
    layer = SoWLinear(20, 12, bias=True, rank=5, n_iter=2, scale=0.5, init_method="normal")
    assert list(layer.state_dict().keys()) == ["acc_upweight", "acc_downweight", "bias", "downscale_weights.0",
                                                "downscale_weights.1", "upscale_weights.0", "upscale_weights.1"]
    assert layer.virtual_rank == 10 and layer.acc_upweight.numel() == 0 and not layer.acc_downweight.requires_grad
    assert isinstance(layer.downscale_weights, SoWParameter) and layer.downscale_weights[0].shape == (20, 5)
    assert layer.upscale_weights[1].shape == (5, 12)
    p0 = layer.downscale_weights[0]
    layer.downscale_weights.from_weights([torch.ones(20, 5), torch.ones(20, 5)])
    assert layer.downscale_weights[0] is p0 and float(p0.data.sum()) == 100.0   # Parameter identity survives
    assert SoWLinear(300, 200, rank=16, n_iter=1, init_method="normal").virtual_rank == 16
    assert "rank=5" in layer.extra_repr()


def test_prepare_sow_names_bit_exact():
    transformers = pytest.importorskip("transformers")
    from sow_amd import SoWConfig, SoWLinear, prepare_sow
    with open(os.path.join(GOLDEN, "prepare_names.json")) as f:
        P = json.load(f)
    cfgs = {
        "llama_60m": transformers.LlamaConfig(hidden_size=512, intermediate_size=1376, num_hidden_layers=8,
                                              num_attention_heads=8, vocab_size=32000, tie_word_embeddings=False),
        "roberta": transformers.RobertaConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                              num_attention_heads=12, vocab_size=50265, max_position_embeddings=514,
                                              type_vocab_size=1),
    }
    for key, cfg in cfgs.items():
        with torch.device("meta"):
            model = transformers.AutoModelForCausalLM.from_config(cfg)
        assert [[n, isinstance(m, nn.Linear)] for n, m in model.named_modules()] == P[key]["named_modules"], key
        model = prepare_sow(model, SoWConfig(target_modules=P[key]["targets"], rank=8, init_method="normal",
                                             decompose=None, device="meta"))
        got = [n for n, m in model.named_modules() if isinstance(m, SoWLinear)]
        assert got == P[key]["replaced"], key
        shapes = {n: [m.in_features, m.out_features, m.virtual_rank] for n, m in model.named_modules()
                  if isinstance(m, SoWLinear)}
        assert shapes == P[key]["shapes"]
    # llama_7b: names only (module tree from the golden file, matching logic from the product)
    from sow_amd.prepare import _is_target
    t7 = P["llama_7b"]["targets"]
    ms = max(len(t.split(".")) for t in t7)
    lin, notlin = nn.Linear(1, 1), nn.Identity()
    got = [n for n, is_lin in P["llama_7b"]["named_modules"] if _is_target(n, lin if is_lin else notlin, t7, ms)]
    assert got == P["llama_7b"]["replaced"] and len(got) == 160


def test_prepare_keep_on_cpu_and_bias_carry():
    from sow_amd import SoWConfig, SoWLinear, prepare_sow
    g = load_golden("prepare_keep")
    m = nn.Sequential()
    m.add_module("fc1", nn.Linear(20, 12, bias=True))
    m.add_module("fc2", nn.Linear(12, 6, bias=False))
    m.fc1.weight.data, m.fc1.bias.data, m.fc2.weight.data = g["w1"], g["b1"], g["w2"]
    bias_obj = m.fc1.bias
    m = prepare_sow(m, SoWConfig(target_modules=["fc1", "fc2"], rank=4, scale=0.5, init_method="normal", decompose="keep",
                                 device="cpu"))
    assert isinstance(m.fc1, SoWLinear) and m.fc1.bias is bias_obj
    assert torch.equal(m.fc1.acc_downweight, g["fc1_acc_down"]) and torch.equal(m.fc2.acc_downweight, g["fc2_acc_down"])
    assert m.fc1.virtual_rank == 12 and m.fc2.virtual_rank == 6 and m.fc1.scale == 0.5
    assert m.fc2.bias is None and m.fc1.acc_upweight.numel() == 0


def test_load_sow_roundtrip(tmp_path):
    from safetensors.torch import save_file

    from sow_amd import SoWLinear, load_sow

    def make():
        net = nn.Sequential()
        net.add_module("a", SoWLinear(10, 8, bias=True, rank=3, init_method="normal"))
        net.add_module("b", SoWLinear(8, 6, bias=False, rank=3, init_method="normal"))
        return net

    torch.manual_seed(0)
    src = make()
    src.a.acc_downweight = nn.Parameter(torch.randn(10, 8), requires_grad=False)            # dense accumulator
    src.b.acc_downweight = nn.Parameter(torch.randn(8, 3), requires_grad=False)             # low-rank accumulator
    src.b.acc_upweight = nn.Parameter(torch.randn(3, 6), requires_grad=False)
    path = str(tmp_path / "model.safetensors")
    save_file({k: v.contiguous() for k, v in src.state_dict().items() if v.numel() > 0}, path)
    dst = make()
    assert dst.a.acc_downweight.numel() == 0
    load_sow(dst, path)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    assert not dst.a.acc_downweight.requires_grad and tuple(dst.b.acc_upweight.shape) == (3, 6)


def test_reset_optimizer_cpu_state_matches_golden():
    from sow_amd import reset_optimizer
    g = load_golden("reset_optimizer")
    ps = [nn.Parameter(torch.zeros(s)) for s in ((6, 4), (4, 3), (3, 5))]
    opt = torch.optim.AdamW([{"params": ps[:1], "lr": 1e-3}, {"params": ps[1:], "lr": 1e-2}])
    for i, p in enumerate(ps):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            v = g[f"before_p{i}_{k}"]
            opt.state[p][k] = v.clone() if torch.is_tensor(v) else torch.tensor(float(v))
    reset_optimizer(opt, group_id=1)
    for i, p in enumerate(ps):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            want = g[f"after_p{i}_{k}"]
            want = want if torch.is_tensor(want) else torch.tensor(float(want))
            assert torch.equal(opt.state[p][k].float(), want.float()), (i, k)


_DP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[3])
rank, world = int(sys.argv[1]), 2
dist.init_process_group("gloo", init_method="file://" + sys.argv[2], rank=rank, world_size=world)
import torch.nn as nn
from sow_amd import SoWLinear, FactorBucket, factor_parameters
torch.manual_seed(0)
net = nn.Sequential(SoWLinear(12, 10, bias=False, rank=4, init_method="normal"), SoWLinear(10, 6, bias=True, rank=4, init_method="normal"))
params = factor_parameters(net)
assert len(params) == 4
before = [p.data.clone() for p in params]
bucket = FactorBucket(params)
assert all(torch.equal(p.data, b) for p, b in zip(params, before))           # re-homing keeps the values
assert all(p.data.data_ptr() >= bucket.flat_param.data_ptr() for p in params)
for i, p in enumerate(params):
    p.grad.fill_(float((rank + 1) * (i + 1)))                                   # writes land in the flat buffer
bucket.all_reduce_async()
scale = bucket.wait()
assert abs(scale - 0.5) < 1e-12
for i, p in enumerate(params):
    assert torch.all(p.grad == 3.0 * (i + 1)), (i, p.grad.flatten()[:3])       # 1x + 2x summed in ONE collective
# accumulate()-style rebinding: new tensors appear, rebind() copies them back into the bucket
params[0].data = torch.full_like(params[0].data, 7.0 + rank)
bucket.rebind()
assert params[0].data.data_ptr() == bucket.flat_param.data_ptr()
bucket.broadcast_factors(src=0)
assert torch.all(params[0].data == 7.0)                                         # rank 1 now holds rank 0's factors
bucket.zero_grad()
assert float(bucket.flat_grad.abs().sum()) == 0.0
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_factor_bucket_allreduce_gloo_world2(tmp_path):
    store = str(tmp_path / "store")
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_DP_WORKER)
    procs = [subprocess.Popen([sys.executable, script, str(r), store, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o


# ---------------------------------------------------------------------------------------------
# the drop-in boundary, as the reference's drivers spell it
# ---------------------------------------------------------------------------------------------
DRIVER_IMPORTS = {
    # file:lines -> the tn_gradient import lines, verbatim
    "scripts/simple_train.py:35-38,45": """
from tn_gradient.optimizer.ttsgd import TTSGD
from tn_gradient.tt import TensorTrain
from tn_gradient.layer.sow import SoWLinear
from tn_gradient.prepare import prepare_sow, accumulate, load_sow, SoWConfig
from tn_gradient.utils import __colorized_str__
""",
    "scripts/finetune.py:32-33": """
from tn_gradient.layer.sow import SoWLinear
from tn_gradient.prepare import prepare_sow, SoWConfig
""",
    "scripts/run_glue.py:55": """
from tn_gradient.prepare import prepare_sow, accumulate, export_alignment
""",
    "scripts/commonsense_evaluate.py:20": """
from tn_gradient.prepare import prepare_sow, SoWConfig
""",
    "scripts/utils/memory_utils.py:3": """
from tn_gradient.layer.sow import SoWLinear
""",
    "tests/tt_adam_update.py:8-9": """
from tn_gradient.tt import TensorTrain
from tn_gradient.utils import closest_factorization, pad_matrix, unpad_matrix
""",
}


@pytest.mark.parametrize("where", list(DRIVER_IMPORTS))
def test_driver_import_lines_resolve_to_sow_amd(where, tmp_path):
    """`simple_train.py` / `finetune.py` unchanged: their tn_gradient imports, executed verbatim in a fresh interpreter with
    the repo first on sys.path, bind the sow_amd implementation."""
    code = ("import sys; sys.path.insert(0, %r)\n" % ROOT) + DRIVER_IMPORTS[where] + """
import sow_amd, tn_gradient
assert tn_gradient.__file__.startswith(%r), tn_gradient.__file__
for name, obj in list(globals().items()):
    if name in ('SoWLinear', 'prepare_sow', 'accumulate', 'load_sow', 'SoWConfig', 'TensorTrain', 'TTSGD'):
        assert obj is getattr(sow_amd, name), name
print('ok')
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_run_glue_sowargs_import_fails_as_in_the_reference():
    """run_glue.py:54 imports `SoWArgs`, which the reference's own tn_gradient/layer/sow.py does not define (SURVEY: the
    script is stale against its library and raises ImportError as shipped).  Same behaviour here -- not papered over."""
    with pytest.raises(ImportError):
        exec("from tn_gradient.layer.sow import SoWLinear, SoWArgs", {})


def test_colorized_str_hook_as_simple_train_installs_it():
    """simple_train.py:45-46: `torch.nn.Module.__str__ = __colorized_str__`.  Children coloured by trainability, runs of
    identical numbered siblings folded into `N x ...` lines."""
    from tn_gradient.utils import __colorized_str__
    from sow_amd import SoWLinear
    from sow_amd.summary import module_summary, trainability
    net = nn.Sequential(nn.Linear(3, 4), nn.ModuleList([nn.Linear(4, 4) for _ in range(4)]), nn.ReLU(),
                        SoWLinear(4, 2, rank=2, init_method="normal"))
    for p in net[1][0].parameters():
        p.requires_grad = False
    text = __colorized_str__(net)
    assert "(1-3): 3 x Linear(in_features=4, out_features=4, bias=True)" in text
    assert "(0): Linear(in_features=4, out_features=4, bias=True)" in text and "SoWLinear(" in text
    assert [trainability(m) for m in (net[0], net[1][0], net[1], net[2], net[3])] == ["trainable", "frozen", "mixed", "none", "mixed"]
    assert "\033[31m(0):\033[0m" in module_summary(net[1], colour=True)          # frozen child in red
    assert "\033[32m(0):\033[0m" in module_summary(net, colour=True)             # trainable child in green
    old = nn.Module.__str__
    try:
        nn.Module.__str__ = __colorized_str__
        assert str(net) == text
    finally:
        nn.Module.__str__ = old


def test_utils_helpers_off_the_hot_path():
    from tn_gradient.utils import generate_rank_k, left_unfolding, perturbe_random, randhaar, randuptri, right_unfolding, unfolding
    t = torch.arange(24.0).reshape(2, 3, 4)
    assert torch.equal(unfolding(t, 1), t.permute(1, 0, 2).reshape(3, 8))
    assert torch.equal(unfolding(t, -1), t.permute(2, 0, 1).reshape(4, 6))
    assert left_unfolding(t).shape == (6, 4) and torch.equal(right_unfolding(t), t.reshape(2, 12))
    with pytest.raises(ValueError):
        unfolding(t, 3)
    q = randhaar(5)
    assert torch.allclose(q @ q.t(), torch.eye(5), atol=1e-5)
    r = randuptri(6)
    assert torch.equal(r, r.triu()) and bool((r.diagonal() > 0).all())
    assert torch.linalg.matrix_rank(generate_rank_k((6, 7), 2)) == 2
    assert perturbe_random(torch.zeros(3, 3)).abs().max() > 0


_DP_PROTOCOL_WORKER = r'''
import copy, os, sys, torch, torch.distributed as dist
root = sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
rank, world = int(sys.argv[1]), 2
dist.init_process_group("gloo", init_method="file://" + sys.argv[2], rank=rank, world_size=world)
import torch.nn as nn
from oracle_backend import OracleSoWLinear           # CPU arithmetic of the layer: the oracle (test infrastructure)
from sow_amd import FactorBucket
from sow_amd.optimizer import FactorAdamW

class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.l1 = OracleSoWLinear(12, 10, False, 4, 0.5, "normal")
        self.l2 = OracleSoWLinear(10, 6, False, 4, 0.5, "normal")
        self.head = nn.Linear(6, 3)
    def forward(self, x):
        return self.head(self.l2(torch.tanh(self.l1(x))))

torch.manual_seed(0)
net = Net()
for m in (net.l1, net.l2):
    nn.init.normal_(m.downscale_weights[0], std=0.3); nn.init.normal_(m.upscale_weights[0], std=0.3)
ref = copy.deepcopy(net)                                 # single-process twin, sees the concatenated batch
X = torch.randn(8, 12)
factors = [net.l1.downscale_weights[0], net.l1.upscale_weights[0], net.l2.downscale_weights[0], net.l2.upscale_weights[0]]
bucket = FactorBucket(factors)                           # CPU-resident flat buffers
ignored = bucket.exclude_from_ddp(net)
assert sorted(ignored) == ["l1.downscale_weights.0", "l1.upscale_weights.0", "l2.downscale_weights.0", "l2.upscale_weights.0"]
ddp = nn.parallel.DistributedDataParallel(net)           # reduces head.* only
bucket._n_attached, bucket._auto = 2, True              # what attach(model, auto_all_reduce=True) sets on the GPU
(ddp(X[4 * rank: 4 * rank + 4]) ** 2).sum().backward()  # autograd accumulates in place into the flat-buffer views
assert not bucket._works
bucket._layer_done()                                     # l2's sink ...
assert not bucket._works
bucket._layer_done()                                     # ... l1's sink: the LAST attached layer issues the all-reduce
assert len(bucket._works) == 1
try:
    bucket._layer_done()                                 # a further backward before wait(): refused, not silently mis-summed
    raise SystemExit("backward during a pending all-reduce was not refused")
except RuntimeError as e:
    assert "no_sync" in str(e)
scale = bucket.wait()
assert abs(scale - 0.5) < 1e-12 and bucket._arrived == 0
(ref(X) ** 2).sum().backward()
ref_f = [ref.l1.downscale_weights[0], ref.l1.upscale_weights[0], ref.l2.downscale_weights[0], ref.l2.upscale_weights[0]]
for p, q in zip(factors, ref_f):
    assert p.grad.data_ptr() == bucket.grad_ptr(p)
    assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-6), (p.grad - q.grad).abs().max()   # SUM over ranks == full batch
assert torch.allclose(net.head.weight.grad, ref.head.weight.grad / world, rtol=1e-5, atol=1e-6)    # DDP averaged the rest
# fused optimizer refuses to step on stale views; accumulate()-style re-init differs per rank until the broadcast
opt = FactorAdamW.__new__(FactorAdamW); opt.bucket = bucket
torch.manual_seed(100 + rank)
for m in (net.l1, net.l2):
    m.next_draws = [torch.randn(m.in_features, m.rank) * 0.02]
    m.accumulate()
try:
    FactorAdamW.step(opt)
    raise SystemExit("stale factor views were not detected")
except RuntimeError as e:
    assert "rebind" in str(e)
bucket.rebind()
assert all(p.data_ptr() == bucket.flat_param.data_ptr() + o * 4 for p, o in zip(bucket.params, bucket.offsets))
mine = net.l1.downscale_weights[0].data.clone()
bucket.broadcast_factors(src=0)
got = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(got, net.l1.downscale_weights[0].data.clone())
assert torch.equal(got[0], got[1])                       # re-initialised A identical on both ranks
assert (rank == 0) == torch.equal(mine, got[0])
assert float(net.l1.upscale_weights[0].abs().max()) == 0.0 and tuple(net.l1.acc_downweight.shape) == (12, 4)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_bucket_protocol_with_ddp_gloo_world2(tmp_path):
    """SURVEY 8e end to end on 2 CPU ranks: factors in the flat bucket (ONE sum all-reduce, issued when the last
    attached layer reports in), everything else through DistributedDataParallel with the factors on its ignore list;
    summed factor gradients == single-process gradients on the concatenated batch; after an accumulate() with
    rank-dependent re-initialisation draws, rebind() + broadcast_factors() make A identical everywhere."""
    store = str(tmp_path / "store")
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_DP_PROTOCOL_WORKER)
    procs = [subprocess.Popen([sys.executable, script, str(r), store, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o


_DP_GA_WORKER = r'''
import copy, os, sys, torch, torch.distributed as dist
root = sys.argv[3]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
rank, world = int(sys.argv[1]), 2
dist.init_process_group("gloo", init_method="file://" + sys.argv[2], rank=rank, world_size=world)
import torch.nn as nn
from oracle_backend import OracleSoWLinear
from sow_amd import FactorBucket

class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.l1 = OracleSoWLinear(12, 10, False, 4, 0.5, "normal")
        self.l2 = OracleSoWLinear(10, 6, False, 4, 0.5, "normal")
        self.head = nn.Linear(6, 3)
    def forward(self, x):
        return self.head(self.l2(torch.tanh(self.l1(x))))

torch.manual_seed(0)
net = Net()
for m in (net.l1, net.l2):
    nn.init.normal_(m.downscale_weights[0], std=0.3); nn.init.normal_(m.upscale_weights[0], std=0.3)
ref = copy.deepcopy(net)
X = torch.randn(8, 12)
factors = [net.l1.downscale_weights[0], net.l1.upscale_weights[0], net.l2.downscale_weights[0], net.l2.upscale_weights[0]]
bucket = FactorBucket(factors)
bucket.exclude_from_ddp(net)
ddp = nn.parallel.DistributedDataParallel(net)
bucket._n_attached, bucket._auto = 2, True              # what attach(model, auto_all_reduce=True) sets on the GPU
mine = X[4 * rank: 4 * rank + 4]
# gradient accumulation = 2 (simple_train.py:596-650): micro-batch 1 local only, micro-batch 2 reduces
with ddp.no_sync(), bucket.no_sync():
    (ddp(mine[:2]) ** 2).sum().backward()
    bucket._layer_done(); bucket._layer_done()
    assert not bucket._works and bucket._arrived == 2
(ddp(mine[2:]) ** 2).sum().backward()
bucket._layer_done()
assert not bucket._works
bucket._layer_done()                                     # 2 micro-batches x 2 layers arrived, armed: ONE collective
assert len(bucket._works) == 1
scale = bucket.wait()
assert abs(scale - 0.5) < 1e-12 and bucket._arrived == 0 and not bucket._works
(ref(X) ** 2).sum().backward()
ref_f = [ref.l1.downscale_weights[0], ref.l1.upscale_weights[0], ref.l2.downscale_weights[0], ref.l2.upscale_weights[0]]
for p, q in zip(factors, ref_f):
    assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-6), (p.grad - q.grad).abs().max()   # both micro-batches of both ranks
assert torch.allclose(net.head.weight.grad, ref.head.weight.grad / world, rtol=1e-5, atol=1e-6)
# every backward disarmed (a loop that forgot to re-arm): wait() still reduces, nothing is lost
bucket.zero_grad()
with ddp.no_sync(), bucket.no_sync():
    (ddp(mine) ** 2).sum().backward()
    bucket._layer_done(); bucket._layer_done()
assert not bucket._works
assert abs(bucket.wait() - 0.5) < 1e-12
for p, q in zip(factors, ref_f):
    assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-6)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_bucket_gradient_accumulation_gloo_world2(tmp_path):
    """Gradient accumulation > 1 with the all-reduce issued from backward: the non-final micro-batches run under
    bucket.no_sync() (and DDP's no_sync()), the final one fires ONE collective over the locally accumulated buffer;
    the result equals the single-process gradient on the concatenated batch of both ranks and both micro-batches."""
    store = str(tmp_path / "store")
    script = str(tmp_path / "worker.py")
    open(script, "w").write(_DP_GA_WORKER)
    procs = [subprocess.Popen([sys.executable, script, str(r), store, ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o


def test_bench_launcher_starts_n_ranks_gloo(tmp_path):
    """`python bench.py --gpus 2` with no torch.distributed environment starts 2 ranks as a child process (config 3's
    launch form, reference readme.md:6 / simple_train.py:229) -- rehearsed on CPU with gloo, stopping after the process
    group is up; a WORLD_SIZE that contradicts --gpus is refused."""
    env = dict(os.environ, SOW_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], capture_output=True,
                         text=True, env=env, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["rccl"] == {"backend": "gloo", "world_size": 2, "ranks_seen": [0, 1]}
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"], capture_output=True,
                         text=True, env=dict(env, WORLD_SIZE="2", RANK="0"), timeout=120, cwd=str(tmp_path))
    assert bad.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in bad.stderr


def test_attach_refuses_a_ddp_wrapped_model_and_optimizer_state_round_trips():
    from sow_amd import FactorBucket, SoWLinear, factor_parameters
    from sow_amd.optimizer import FactorAdamW
    net = nn.Sequential(SoWLinear(12, 10, bias=False, rank=4, init_method="normal"))
    bucket = FactorBucket(factor_parameters(net))

    class FakeDDP(torch.nn.parallel.DistributedDataParallel):
        def __init__(self):       # no process group needed for the isinstance check
            nn.Module.__init__(self)

    with pytest.raises(RuntimeError, match="exclude_from_ddp"):
        bucket.attach(FakeDDP())
    opt = FactorAdamW(bucket, lr=3e-3, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.1, state_dtype=torch.float32)
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    opt.step_count = 7
    opt.param_groups[0]["lr"] = 1e-3            # what an LR scheduler does
    sd = opt.state_dict()
    assert sd["lr"] == 1e-3 and opt.lr == 1e-3  # the written value is the one saved (and the one the next step() uses)
    assert opt.param_groups[0]["lr"] == 1e-3
    other = FactorAdamW(bucket, state_dtype=torch.float32)
    other.load_state_dict(opt.state_dict())
    assert other.step_count == 7 and other.lr == 1e-3 and other.betas == (0.9, 0.95) and other.weight_decay == 0.1
    assert torch.equal(other.exp_avg, opt.exp_avg) and torch.equal(other.exp_avg_sq, opt.exp_avg_sq)
    with pytest.raises(ValueError):
        FactorAdamW(FactorBucket([nn.Parameter(torch.zeros(5))])).load_state_dict(sd)


def test_group_slab_plan_is_a_pure_function_of_the_layer_list():
    """sow_backward_group_plan (host logic only, no launch): the seven projections of a llama_60m decoder block plan to one
    resident round of equal-work blocks for the row-owner weight-gradient kernel (13 slabs for the 512-wide operands, 18 per
    column range for the 1376-wide ones: 251 blocks); three q / k / v layers do not fill the chip and keep the single-layer
    slab counts; a deferred reduction (PARTIAL alone) keeps them too unless SOW_BWD_GROUP_SLABS is passed; short inputs
    (llama-7b fine-tuning, T = 1024) never qualify."""
    from sow_amd import _lib
    lib = _lib.load()

    def layer(T, d_in, d_out, r=50):
        ws = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, 0, _lib.BF16)
        fake = 1 << 20     # the plan looks at alignment and sizes only; nothing is dereferenced
        return _lib.LayerArgs(x=fake, A=fake, B=fake, y=fake, h_save=fake, dy=fake, dx=fake, dA=fake, dB=fake, T=T, d_in=d_in,
                              d_out=d_out, r_live=r, r_acc=0, acc_kind=0, scale=1.0, grad_beta=0.0, workspace=fake,
                              workspace_bytes=ws + 256)

    def plan(layers, phases):
        arr = (_lib.LayerArgs * len(layers))(*layers)
        slabs = (ctypes.c_int * (2 * len(layers)))()
        return lib.sow_backward_group_plan(arr, len(layers), _lib.BF16, phases, slabs), list(slabs)

    block = [layer(32768, 512, 512)] * 4 + [layer(32768, 512, 1376)] * 2 + [layer(32768, 1376, 512)]
    full = _lib.BWD_DATA | _lib.BWD_WEIGHTS
    rows, slabs = plan(block, full)
    assert rows == 1 and slabs == [13] * 9 + [18, 13, 18, 18, 13]
    assert sum(n * (2 if i in (9, 11, 12) else 1) for i, n in enumerate(slabs)) == 251
    assert plan(block, _lib.BWD_WEIGHTS_PARTIAL) == (0, [32] * 8 + [16] * 6)
    assert plan(block, _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS) == (1, slabs)
    assert plan(block, _lib.BWD_WEIGHTS_REDUCE | _lib.BWD_GROUP_SLABS) == (1, slabs)
    assert plan(block, _lib.BWD_DATA)[0] == 0
    assert plan(block[:3], full) == (0, [32] * 6)
    assert plan([layer(1024, 4096, 4096, 8)] * 3 + [layer(1024, 4096, 11008, 8), layer(1024, 11008, 4096, 8)], full)[0] == 0
    # an unaligned input pointer or a workspace sized by an older rule: no row-owner kernel, never an error
    odd = layer(32768, 512, 512)
    odd.x = (1 << 20) + 8
    assert plan(block[:6] + [odd], full)[0] == 0
    small = layer(32768, 1376, 512)
    small.workspace_bytes = 1 << 20
    assert plan(block[:6] + [small], full)[0] == 0
