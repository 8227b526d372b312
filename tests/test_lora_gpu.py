"""LoRA adapters on the GPU (-m gpu): the four kernels of csrc/lora.hip, the
LoraCausalLM forward / backward, the merged-weights rollout and
GRPOTrainer(peft_config=...).

Kernel comparisons are against a float64 reference computed from the same bf16
inputs (for up_add and the gradients, from u as stored in bf16).  The bound is
derived, not measured:

    |out - ref| <= 2^-8 |ref| + L 2^-23 sum|terms|

L the reduction length (the added-to value counts as one term); the first term
is one bf16 rounding with a factor 2 and is dropped for fp32 outputs, the second
is the worst-case fp32 accumulation error of L terms in any order.

Model and trainer comparisons are against transformers Qwen2ForCausalLM /
LlamaForCausalLM whose target Linears are wrapped in a plain-torch LoRA Linear
(`_OracleLora`: base(x) + s B(A(x))), with the bounds of
tests/test_step_parity_gpu.py (`_check_fp32`, `_check_bf16`).
"""
import json
import multiprocessing as mp
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EOS, PAD = 1, 0


def _randn(shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def _rank_matrix(r, cols, seed, scale=1.0):
    """[Rp, cols] bf16 with rows >= r zero (the storage convention)."""
    from swh_trl_amd import nn_ops
    m = _randn((nn_ops.lora_rank_pad(r), cols), seed, scale)
    m[r:] = 0
    return m


def _rank_cols(T, r, seed):
    """u [T, Rp] bf16 with columns >= r zero (what lora_down writes)."""
    from swh_trl_amd import nn_ops
    u = _randn((T, nn_ops.lora_rank_pad(r)), seed)
    u[:, r:] = 0
    return u


def _within(out, ref, terms, L, bf16_out):
    """The module docstring's bound, elementwise."""
    bound = L * 2.0 ** -23 * terms + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    err = (out.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))


def _window(T, C, seed, left=32, right=64, scale=1.0):
    """A [T, C] column window (nonzero offset, ld > C) of a wider random bf16 buffer."""
    buf = _randn((T, left + C + right), seed, scale)
    return buf, buf[:, left:left + C]


# --------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("T", [1, 63, 200])
@pytest.mark.parametrize("K,r", [(256, 4), (256, 8), (896, 16), (512, 64)])
def test_lora_down(T, K, r):
    from swh_trl_amd import nn_ops
    _, x = _window(T, K, 1)
    assert x.stride(0) > K
    M = _rank_matrix(r, K, 2, K ** -0.5)
    u = nn_ops.lora_down(x, M, r)
    assert u.shape == (T, nn_ops.lora_rank_pad(r)) and u.dtype == torch.bfloat16
    ref = x.double() @ M.double().t()
    _within(u, ref, x.double().abs() @ M.double().abs().t(), K, True)
    assert not bool(u[:, r:].any())  # pad columns exactly zero
    assert bool(u[:, :r].any())


@pytest.mark.parametrize("T", [1, 63, 200])
@pytest.mark.parametrize("C", [128, 896])
@pytest.mark.parametrize("r,s", [(8, 2.0), (40, 0.0625), (64, 2.0), (16, 0.0625)])
def test_lora_up_add(T, C, r, s):
    from swh_trl_amd import nn_ops
    buf, y = _window(T, C, 3)
    before = buf.clone()
    u, M = _rank_cols(T, r, 4), _rank_matrix(r, C, 5, 0.25)
    Rp = M.shape[0]
    nn_ops.lora_up_add(y, u, M, r, s)
    y0 = before[:, 32:32 + C].double()
    ref = y0 + s * (u.double() @ M.double())
    _within(y, ref, y0.abs() + s * (u.double().abs() @ M.double().abs()), Rp + 1, True)
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:, 32:32 + C] = False
    assert torch.equal(buf.view(torch.int16)[outside], before.view(torch.int16)[outside])
    assert not torch.equal(buf, before)
    # a zero M leaves y as it was
    buf2 = before.clone()
    nn_ops.lora_up_add(buf2[:, 32:32 + C], u, torch.zeros_like(M), r, s)
    assert torch.equal(buf2, before)


@pytest.mark.parametrize("T", [1, 200, 8229])
@pytest.mark.parametrize("C", [256, 896])
@pytest.mark.parametrize("r", [8, 64])
def test_lora_grad(T, C, r):
    from swh_trl_amd import nn_ops
    s = 0.5
    _, x = _window(T, C, 6)
    u = _rank_cols(T, r, 7)
    Rp = u.shape[1]
    G0 = _randn((Rp, C), 8, dtype=torch.float32)
    G0[r:] = 0
    G = G0.clone()
    nn_ops.lora_grad(G, u, x, r, s)
    ref = G0.double() + s * (u.double().t() @ x.double())
    _within(G, ref, G0.double().abs() + s * (u.double().abs().t() @ x.double().abs()), T + 1, False)
    assert not torch.equal(G, G0)
    assert not bool(G[r:].any())  # pad rows exactly zero
    G2 = G0.clone()
    nn_ops.lora_grad(G2, u, x, r, s)  # no atomics: a second run gives the same bits
    assert torch.equal(G2.view(torch.int32), G.view(torch.int32))


def test_lora_merge_two_jobs():
    from swh_trl_amd import nn_ops
    jobs, keep = [], []
    for j, ((N, K), r, s) in enumerate(zip([(128, 256), (1024, 256)], [8, 40], [2.0, 0.0625])):
        W = _randn((N, K), 10 + j, 0.05)
        A, Bt = _rank_matrix(r, K, 20 + j, K ** -0.5), _rank_matrix(r, N, 30 + j, 0.05)
        keep.append((W, A, Bt, r, s))
        jobs.append((W, A, Bt, torch.full_like(W, 7.0), r, s))
    nn_ops.lora_merge(*nn_ops.lora_merge_table(jobs, DEV))
    for (W, A, Bt, r, s), job in zip(keep, jobs):
        out = job[3]
        ref = W.double() + s * (Bt.double().t() @ A.double())
        _within(out, ref, W.double().abs() + s * (Bt.double().abs().t() @ A.double().abs()), A.shape[0] + 1, True)
        assert not torch.equal(out, W)
    # Bt = 0: the output bits are W's
    zjobs = [(W, A, torch.zeros_like(Bt), torch.full_like(W, 7.0), r, s) for (W, A, Bt, r, s) in keep]
    nn_ops.lora_merge(*nn_ops.lora_merge_table(zjobs, DEV))
    for (W, *_), job in zip(keep, zjobs):
        assert torch.equal(job[3].view(torch.int16), W.view(torch.int16))


def test_lora_argument_errors_raise_before_any_launch():
    from swh_trl_amd import _lib, nn_ops
    x, M, u = _randn((16, 256), 1), _rank_matrix(8, 256, 2), torch.zeros(16, 16, device=DEV, dtype=torch.bfloat16)
    dt, st = _lib.dtype_code(x, "test"), torch.cuda.current_stream().cuda_stream

    def down(xp=None, T=16, K=256, r=8, ldx=256, ldm=256, ldu=16):
        _lib.call("swh_lora_down", x.data_ptr() if xp is None else xp, M.data_ptr(), u.data_ptr(), T, K, r, ldx, ldm,
                  ldu, dt, st)

    down()  # the valid call
    u_valid = u.clone()
    for bad in (dict(r=65), dict(r=0), dict(K=48), dict(ldx=257), dict(ldu=12), dict(xp=x.data_ptr() + 2),
                dict(ldx=128)):
        with pytest.raises(ValueError):
            down(**bad)
    y = torch.zeros(16, 128, device=DEV, dtype=torch.bfloat16)
    Mu = _rank_matrix(8, 128, 3)
    for bad in (dict(r=65), dict(C=120), dict(ldy=129), dict(yp=y.data_ptr() + 2)):
        kw = dict(yp=y.data_ptr(), C=128, r=8, ldy=128)
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.call("swh_lora_up_add", u.data_ptr(), Mu.data_ptr(), kw["yp"], 16, kw["C"], kw["r"], 16, 128,
                      kw["ldy"], 1.0, dt, st)
    G = torch.zeros(16, 128, device=DEV)
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    for bad in (dict(r=65), dict(C=120), dict(ldin=129), dict(wsb=16)):
        kw = dict(C=128, r=8, ldin=128, wsb=ws.numel())
        kw.update(bad)
        with pytest.raises(ValueError):
            _lib.call("swh_lora_grad", u.data_ptr(), y.data_ptr(), G.data_ptr(), 16, kw["C"], kw["r"], 16, kw["ldin"],
                      128, 1.0, dt, ws.data_ptr(), kw["wsb"], st)
    with pytest.raises(ValueError):  # an fp32 buffer is refused by its dtype code
        xf = x.float()
        _lib.call("swh_lora_down", xf.data_ptr(), M.data_ptr(), u.data_ptr(), 16, 256, 8, 256, 256, 16,
                  _lib.dtype_code(xf, "test"), st)
    with pytest.raises(ValueError):
        _lib.call("swh_lora_merge", None, 1, 1, st)
    # the wrappers refuse the same shapes
    with pytest.raises(ValueError):
        nn_ops.lora_down(x, _randn((80, 256), 4), 65)
    with pytest.raises(ValueError):
        nn_ops.lora_down(x[:, :48], M[:, :48], 8)
    with pytest.raises(ValueError):
        nn_ops.lora_down(x[:, 1:33], M[:, :32], 8)  # misaligned base
    torch.cuda.synchronize()
    assert torch.equal(u, u_valid) and not bool(y.any()) and not bool(G.any())  # none of the refused calls wrote


# --------------------------------------------------------------------------- the transformers oracle
class _OracleLora(torch.nn.Module):
    """peft's LoRA Linear in plain torch: base(x) + s B(A(x)), base frozen."""

    def __init__(self, base, r, scale):
        super().__init__()
        kw = dict(bias=False, dtype=base.weight.dtype, device=base.weight.device)
        self.base, self.scale = base, scale
        self.lora_A = torch.nn.Linear(base.in_features, r, **kw)
        self.lora_B = torch.nn.Linear(r, base.out_features, **kw)

    def forward(self, x):
        return self.base(x) + self.scale * self.lora_B(self.lora_A(x))


def _oracle(cfg, base_sd, spec, adapter_sd, dtype, device="cpu"):
    """transformers model with the base weights, every target wrapped, the adapter loaded
    from its peft-named state dict; only the adapter parameters require grad."""
    from oracle import grpo_step as og
    hf = og.hf_from_config(cfg.to_dict(), seed=0, dtype=dtype).to(device)
    missing, unexpected = hf.load_state_dict({k: v.to(dtype) for k, v in base_sd.items()}, strict=False)
    assert not unexpected and not [k for k in missing if "rotary" not in k], (missing, unexpected)
    for p in hf.parameters():
        p.requires_grad_(False)
    if spec is None:
        return hf
    for i, layer in enumerate(hf.model.layers):
        for m in spec.targets:
            parent = layer.self_attn if m in ("q_proj", "k_proj", "v_proj", "o_proj") else layer.mlp
            w = _OracleLora(getattr(parent, m), spec.r, spec.scale)
            pre = f"base_model.model.model.layers.{i}.{'self_attn' if parent is layer.self_attn else 'mlp'}.{m}."
            with torch.no_grad():
                w.lora_A.weight.copy_(adapter_sd[pre + "lora_A.weight"])
                w.lora_B.weight.copy_(adapter_sd[pre + "lora_B.weight"])
            setattr(parent, m, w)
    return hf


def _peft_named(named):
    return {"base_model.model." + n: t for n, t in named}


def _lora_model(cfg, spec, dtype, b_std=0.02, seed=3, std=0.05):
    """LoraCausalLM with random base weights and B ~ N(0, b_std) (A as initialised)."""
    from swh_trl_amd.engine import LoraCausalLM
    m = LoraCausalLM(cfg, torch.device(DEV), spec, dtype=dtype, seed=seed, adapter_seed=5, init_std=std)
    sd = m.adapter_state_dict()
    g = torch.Generator().manual_seed(9)
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * b_std
    m.load_adapter_state_dict(sd)
    return m


def _cpu(sd):
    return {k: v.detach().float().cpu().clone() for k, v in sd.items()}


def _engine_logp_and_grads(m, ids, km, w):
    m.zero_grad()
    h = m.hidden_states(ids, key_mask=km)
    lp, _ = m.logp_entropy(h[:, :-1], ids[:, 1:], 1.0, False)
    (lp * w).sum().backward()
    torch.cuda.synchronize()
    return lp.detach().float().cpu(), _cpu(m.adapter_grad_state_dict())


def _oracle_logp_and_grads(hf, ids, km, w):
    from oracle import trl_ref
    logits = hf(input_ids=ids.cpu(), attention_mask=km.cpu().long()).logits[:, :-1]
    lp = trl_ref.selective_log_softmax(logits, ids[:, 1:].cpu())
    (lp.float() * w.cpu()).sum().backward()
    return lp.detach().float(), _cpu(_peft_named((n, p.grad) for n, p in hf.named_parameters() if p.grad is not None))


def _model_cases():
    from swh_trl_amd.engine import tiny_llama, tiny_qwen2
    # r 8: the stacked qkv A (48 rows) goes through one kernel call; r 20: Rp 32, the stack of 96 rows per slice
    return [("qwen2", tiny_qwen2(1024, 2), 8), ("llama", tiny_llama(2048, 2), 20)]


@pytest.fixture(scope="module", params=_model_cases(), ids=lambda c: c[0])
def grad_case(request):
    """One architecture: inputs, and the fp32 oracle's log-probs / gradients (shared by both precisions)."""
    from swh_trl_amd.engine import LoraConfig, lora
    name, cfg, r = request.param
    spec = lora.resolve(LoraConfig(r=r, lora_alpha=2 * r, target_modules="all-linear"), cfg.model_type)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(2, cfg.vocab_size, (4, 24), generator=g)
    km = torch.ones(4, 24, dtype=torch.int32)
    km[0, :5] = 0
    km[1, :3] = 0
    ids[km == 0] = PAD
    w = torch.randn(4, 23, generator=g) * (km[:, 1:] * km[:, :-1])
    # the bf16 model defines the weights (bf16 values), so every run sees the same numbers
    mb = _lora_model(cfg, spec, torch.bfloat16)
    base, adapter = _cpu(mb.hf_state_dict()), _cpu(mb.adapter_state_dict())
    lp32, g32 = _oracle_logp_and_grads(_oracle(cfg, base, spec, adapter, torch.float32), ids, km, w)
    return dict(cfg=cfg, spec=spec, ids=ids.to(DEV), km=km.to(DEV), w=w.to(DEV), mb=mb, base=base, adapter=adapter,
                lp32=lp32, g32=g32, valid=(km[:, 1:] * km[:, :-1]).bool())


def test_model_gradients_fp32(grad_case):
    from swh_trl_amd.engine import LoraCausalLM
    c = grad_case
    m = LoraCausalLM(c["cfg"], torch.device(DEV), c["spec"], dtype=torch.float32, seed=None)
    m.load_hf_state_dict({k: v.to(DEV) for k, v in c["base"].items()})
    m.load_adapter_state_dict(c["adapter"])
    assert not m._hip_lora
    lp, grads = _engine_logp_and_grads(m, c["ids"], c["km"], c["w"])
    assert (lp - c["lp32"]).abs()[c["valid"]].max().item() <= 1e-4
    assert set(grads) == set(c["g32"]) == set(c["adapter"])
    for k, g32 in c["g32"].items():
        rel = ((grads[k] - g32).norm() / g32.norm().clamp_min(1e-20)).item()
        assert rel <= 1e-3, (k, rel)
    assert m.grad is None  # the base has no gradient buffer


def test_model_gradients_bf16(grad_case):
    from test_step_parity_gpu import _ulp_bf16
    c = grad_case
    m = c["mb"]
    assert m._hip_lora
    lp, grads = _engine_logp_and_grads(m, c["ids"], c["km"], c["w"])
    lpb, gb = _oracle_logp_and_grads(_oracle(c["cfg"], c["base"], c["spec"], c["adapter"], torch.bfloat16), c["ids"],
                                     c["km"], c["w"])
    v = c["valid"]
    d_ref, d_pb = (lpb - c["lp32"]).abs()[v], (lp - lpb).abs()[v]
    ulp = _ulp_bf16(lpb.abs().max().item())
    print("logp: ref", d_ref.max().item(), d_ref.mean().item(), "product", d_pb.max().item(), d_pb.mean().item())
    assert d_pb.max().item() <= 2 * d_ref.max().item() + ulp
    assert d_pb.mean().item() <= 2 * d_ref.mean().item() + ulp / 2
    for k, g32 in c["g32"].items():
        n32 = g32.norm().clamp_min(1e-20)
        rel_ref, rel_p = ((gb[k] - g32).norm() / n32).item(), ((grads[k] - g32).norm() / n32).item()
        print(k, rel_p, rel_ref)
        assert rel_p <= 2 * rel_ref + 2.0 ** -8, (k, rel_p, rel_ref)
    # pad rows of the gradient buffer stay exactly zero
    r, Rp = c["spec"].r, c["spec"].rank_pad
    for name, t in m.ga.items():
        for r0 in range(0, t.shape[0], Rp):
            assert not bool(t[r0 + r:r0 + Rp].any()), name
    # the torch composition (EngineOptions.hip_lora False) computes the same thing
    m.options = m.options.replace(hip_lora=False)
    try:
        lp_t, grads_t = _engine_logp_and_grads(m, c["ids"], c["km"], c["w"])
    finally:
        m.options = m.options.replace(hip_lora=True)
    for k, g32 in c["g32"].items():
        n32 = g32.norm().clamp_min(1e-20)
        assert ((grads_t[k] - g32).norm() / n32).item() <= 2 * ((gb[k] - g32).norm() / n32).item() + 2.0 ** -8, k


def test_adapters_disabled_is_the_base_model_bit_for_bit():
    from swh_trl_amd.engine import CausalLM, LoraConfig, lora, tiny_qwen2
    cfg = tiny_qwen2(1024, 2)
    spec = lora.resolve(LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"))
    m = _lora_model(cfg, spec, torch.bfloat16)
    plain = CausalLM(cfg, torch.device(DEV), seed=None, trainable=False)
    plain.copy_from(m)
    ids = torch.randint(2, 1024, (4, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        want = plain.logits(plain.hidden_states(ids))
        on = m.logits(m.hidden_states(ids))
        with m.adapters_disabled():
            off = m.logits(m.hidden_states(ids))
        on2 = m.logits(m.hidden_states(ids))
    assert torch.equal(off.view(torch.int16), want.view(torch.int16))
    assert not torch.equal(on, want) and torch.equal(on, on2)


def test_decode_reads_the_merged_weights(tmp_path):
    from swh_trl_amd.engine import CausalLM, DecodeEngine, LoraConfig, lora, tiny_qwen2
    from swh_trl_amd.trainer import checkpoint as ck
    from swh_trl_amd.trainer.grpo_trainer import load_model
    cfg = tiny_qwen2(1024, 2)
    spec = lora.resolve(LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"))
    m = _lora_model(cfg, spec, torch.bfloat16, b_std=0.05)
    g = torch.Generator().manual_seed(2)
    pid = torch.randint(2, 1024, (8, 8), generator=g).to(DEV)
    pm = torch.ones(8, 8, dtype=torch.int32, device=DEV)

    def greedy(model):
        eng = DecodeEngine(model, 8, 8, 16)
        out, _ = eng.generate(pid, pm, 16, greedy=True, pad_token_id=PAD)
        return out.clone()

    ids_lora = greedy(m.decode_view())
    ck.save_pretrained(m, str(tmp_path), state_dict=m.merged_hf_state_dict())
    merged = load_model(str(tmp_path), torch.device(DEV), trainable=False)
    base = CausalLM(cfg, torch.device(DEV), seed=None, trainable=False)
    base.copy_from(m)
    ids_merged, ids_base = greedy(merged), greedy(base)
    assert bool((ids_merged != ids_base).any(1).any())  # the adapter is large enough to change the rollout
    assert torch.equal(ids_lora, ids_merged)
    # untargeted tensors alias the base, targets are copies
    view = m.decode_view()
    assert view.p["embed"].data_ptr() == m.p["embed"].data_ptr()
    assert view.p["l0.qkv_w"].data_ptr() != m.p["l0.qkv_w"].data_ptr()


# --------------------------------------------------------------------------- trainer
def _reward_product(prompts=None, completions=None, completion_ids=None, **kw):
    return [float(sum(c) % 7) for c in completion_ids]


def _reward_oracle(cids, cmask):
    return [float(sum(r[m.bool()].tolist()) % 7) for r, m in zip(cids, cmask)]


def _dataset(cfg, n, P, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [{"prompt": None, "prompt_ids": torch.randint(2, cfg.vocab_size, (P,), generator=g).tolist()}
            for _ in range(n)]


def _trainer(cfg, dtype, peft_config, *, n_steps, P=16, C=16, MB=8, GA=1, G=4, beta=0.04, lr=1e-3, out=None,
             min_new_tokens=4, **kw):
    from swh_trl_amd.engine import CausalLM
    from swh_trl_amd.trainer import GRPOConfig, GRPOTrainer
    args = GRPOConfig(output_dir=out, per_device_train_batch_size=MB, gradient_accumulation_steps=GA,
                      num_generations=G, max_prompt_length=P, max_completion_length=C, learning_rate=lr,
                      max_steps=n_steps, lr_scheduler_type="constant", seed=5, shuffle_dataset=False, beta=beta,
                      model_init_kwargs={"torch_dtype": "float32" if dtype == torch.float32 else "bfloat16"},
                      generation_kwargs={"eos_token_id": EOS, "pad_token_id": PAD, "min_new_tokens": min_new_tokens},
                      **kw)
    model = CausalLM(cfg, torch.device(DEV), seed=3, init_std=0.05, dtype=dtype, trainable=False)
    ds = _dataset(cfg, MB * GA // G * max(1, n_steps), P)
    return GRPOTrainer(model=model, reward_funcs=_reward_product, args=args, train_dataset=ds,
                       peft_config=peft_config)


def test_trainer_trains_the_adapter_only():
    from swh_trl_amd.engine import LoraCausalLM, LoraConfig, tiny_qwen2
    cfg = tiny_qwen2(1024, 2)
    tr = _trainer(cfg, torch.bfloat16, LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"), n_steps=3)
    assert isinstance(tr.model, LoraCausalLM) and tr.ref_model is None and tr.model.grad is None
    assert tr.optimizer.numel == tr.model.adapter_numel and tr.optimizer.no_decay is None
    base0 = tr.model.flat.clone()
    met = []
    for _ in range(3):
        tr.training_step_group()
        torch.cuda.synchronize()
        met.append(tr._metrics["train"]["_met"][-1].detach().cpu().clone())
    # step 1: B = 0, so the policy is the base model: KL exactly 0, nothing clipped
    assert torch.all(met[0][:, 0] > 0) and torch.all(met[0][:, 1] == 0) and torch.all(met[0][:, 3:6] == 0), met[0]
    assert float(met[2][:, 1].sum()) > 0, met[2]
    assert torch.equal(tr.model.flat.view(torch.int16), base0.view(torch.int16))
    sd = tr.model.adapter_state_dict()
    assert len(sd) == 2 * 7 * cfg.num_hidden_layers
    for k, t in sd.items():
        assert torch.isfinite(t.float()).all(), k
        if "lora_B" in k:
            assert bool(t.any()), k
    r, Rp = tr.lora.r, tr.lora.rank_pad
    for name, t in tr.model.a.items():  # pad rows stay exactly zero under training
        for r0 in range(0, t.shape[0], Rp):
            assert not bool(t[r0 + r:r0 + Rp].any()), name
    assert not bool(tr.optimizer.master.isnan().any())


def test_trainer_refusals():
    from swh_trl_amd.engine import LoraConfig, gpt2_config, tiny_qwen2
    from swh_trl_amd.trainer import GRPOConfig, GRPOTrainer
    with pytest.raises(ValueError, match="sync_ref_model"):
        _trainer(tiny_qwen2(1024, 2), torch.bfloat16, LoraConfig(), n_steps=1, sync_ref_model=True)
    with pytest.raises(ValueError, match="use_dora"):
        _trainer(tiny_qwen2(1024, 2), torch.bfloat16, LoraConfig(use_dora=True), n_steps=1)
    args = GRPOConfig(output_dir=None, per_device_train_batch_size=8, num_generations=4, max_prompt_length=8,
                      max_completion_length=8)
    with pytest.raises(ValueError, match="gpt2"):
        GRPOTrainer(model=gpt2_config(), reward_funcs=_reward_product, args=args, train_dataset=[],
                    peft_config=LoraConfig())


def _randomize_b(tr, std=0.02):
    """B ~ N(0, std) in the trainer's model and optimizer master (the same on every rank)."""
    sd = tr.model.adapter_state_dict()
    g = torch.Generator().manual_seed(9)
    for k in sd:
        if "lora_B" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * std
    tr.model.load_adapter_state_dict(sd)
    tr.optimizer.master.copy_(tr.model.adapter.float())


def _lora_product_run(cfg, dtype, peft_config, lr, beta, GA=2):
    """One optimizer step of GRPOTrainer(peft_config=...), captured as
    tests/test_step_parity_gpu.py product_run captures it (names are peft's)."""
    tr = _trainer(cfg, dtype, peft_config, n_steps=1, P=12, C=24, MB=8, GA=GA, beta=beta, lr=lr)
    _randomize_b(tr)  # B = 0 would leave dA = 0 and the policy equal to the reference
    base, a0 = _cpu(tr.model.hf_state_dict()), _cpu(tr.model.adapter_state_dict())
    cap = {"gens": [], "logps": [], "masks": []}
    gen_fn, lp_fn = tr._generate_and_score_completions, tr._completion_logps

    def gen_capture(examples):
        out = gen_fn(examples)
        rec = {k: v.detach().cpu().clone() for k, v in out.items()}
        rec["perm"] = torch.randperm(rec["completion_ids"].shape[0],
                                     generator=torch.Generator().set_state(tr._shuffle_gen.get_state()))
        cap["gens"].append(rec)
        return out

    def lp_capture(model_, batch, compute_entropy):
        lp, ent = lp_fn(model_, batch, compute_entropy)
        if compute_entropy:
            cap["logps"].append(lp.detach().float().cpu().clone())
            cap["masks"].append(batch["completion_mask"].detach().cpu().clone())
        return lp, ent

    tr._generate_and_score_completions, tr._completion_logps = gen_capture, lp_capture
    out = tr.training_step_group()
    torch.cuda.synchronize()
    step = {"loss": float(out["loss"]), "grad_norm": float(out["grad_norm"]),
            "grads": _cpu(tr.model.adapter_grad_state_dict()), "w": _cpu(tr.model.adapter_state_dict()),
            "logps": cap["logps"][-1], "mask": cap["masks"][-1],
            "seg_metrics": tr._metrics["train"]["_met"][-1].detach().cpu().clone()}
    return {"w0": a0, "base": base, "gens": cap["gens"], "steps": [step], "spec": tr.lora,
            "geometry": dict(G=4, C=24, MB=8, GA=GA)}


def _lora_oracle_run(cfg, prod, dtype, lr, beta):
    from oracle import grpo_step as og
    geo = prod["geometry"]
    hf = _oracle(cfg, prod["base"], prod["spec"], prod["w0"], dtype)
    ref = _oracle(cfg, prod["base"], None, None, dtype)  # the frozen base: the adapter switched off
    params = [p for p in hf.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, foreach=False)
    gens = [{"prompt_ids": g["prompt_ids"], "prompt_mask": g["prompt_mask"].long(),
             "completion_ids": g["completion_ids"], "perm": g["perm"]} for g in prod["gens"]]
    recs = og.grpo_train(hf, opt, gens, _reward_oracle, num_generations=geo["G"], C=geo["C"],
                         per_device_train_batch_size=geo["MB"], gradient_accumulation_steps=geo["GA"], n_steps=1,
                         eos_token_id=EOS, beta=beta, ref_model=ref, capture=True)
    for r in recs:
        r["grads"] = _peft_named((k, v.float()) for k, v in r["grads"].items())
    recs[0]["w_after"] = _peft_named((k, p.detach().float().cpu().clone()) for k, p in hf.named_parameters()
                                     if p.requires_grad)
    return recs


def test_trainer_step_matches_oracle_fp32():
    from test_step_parity_gpu import _check_fp32
    from swh_trl_amd.engine import LoraConfig, tiny_qwen2
    cfg, lr, beta = tiny_qwen2(1024, 2), 1e-3, 0.04
    prod = _lora_product_run(cfg, torch.float32, LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"), lr, beta)
    orc = _lora_oracle_run(cfg, prod, torch.float32, lr, beta)
    assert set(orc[0]["grads"]) == set(prod["steps"][0]["grads"]) == set(prod["w0"])
    _check_fp32("lora-fp32", prod, orc, lr)


def test_trainer_step_matches_oracle_bf16():
    from test_step_parity_gpu import _check_bf16
    from swh_trl_amd.engine import LoraConfig, tiny_qwen2
    cfg, lr, beta = tiny_qwen2(1024, 2), 1e-3, 0.04
    prod = _lora_product_run(cfg, torch.bfloat16, LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"), lr, beta)
    orc_bf = _lora_oracle_run(cfg, prod, torch.bfloat16, lr, beta)
    orc_32 = _lora_oracle_run(cfg, prod, torch.float32, lr, beta)
    # B != 0 here, so the step-1 KL is not 0 (test_trainer_trains_the_adapter_only pins that case): beta=0.0
    # only switches that assertion of _check_bf16 off; both sides train with beta 0.04
    assert float(prod["steps"][0]["seg_metrics"][:, 1].sum()) > 0
    _check_bf16("lora-bf16", prod, orc_bf, orc_32, beta=0.0)


def test_checkpoint_resume_and_adapter_files(tmp_path):
    from safetensors.torch import load_file
    from swh_trl_amd.engine import LoraConfig, lora, tiny_qwen2
    cfg = tiny_qwen2(1024, 2)
    pc = LoraConfig(r=8, lora_alpha=16, target_modules=["q_proj", "v_proj", "down_proj"])
    kw = dict(n_steps=3, save_strategy="steps", logging_steps=1)
    full = _trainer(cfg, torch.bfloat16, pc, out=str(tmp_path / "a"), save_steps=1, **kw)
    full.train()
    d = tmp_path / "a" / "checkpoint-2"
    sd = load_file(str(d / "adapter_model.safetensors"))
    want = {lora.peft_key(i, m, w) for i in range(2) for m in ("q_proj", "v_proj", "down_proj") for w in "AB"}
    assert set(sd) == want and not (d / "model.safetensors").exists()
    assert sd["base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"].shape == (8, cfg.hidden_size)
    assert sd["base_model.model.model.layers.1.self_attn.v_proj.lora_B.weight"].shape == (cfg.kv_dim, 8)
    assert sd["base_model.model.model.layers.1.mlp.down_proj.lora_A.weight"].shape == (8, cfg.intermediate_size)
    conf = json.loads((d / "adapter_config.json").read_text())
    assert conf["peft_type"] == "LORA" and conf["r"] == 8 and conf["lora_alpha"] == 16
    assert conf["target_modules"] == ["q_proj", "v_proj", "down_proj"] and conf["lora_dropout"] == 0.0
    assert conf["bias"] == "none" and conf["task_type"] == "CAUSAL_LM" and "base_model_name_or_path" in conf
    res = _trainer(cfg, torch.bfloat16, pc, out=str(tmp_path / "b"), save_steps=10 ** 9, **kw)
    res.train(resume_from_checkpoint=str(d))
    assert res.state.global_step == 3
    torch.cuda.synchronize()
    assert torch.equal(res.model.adapter.view(torch.int16), full.model.adapter.view(torch.int16))
    assert torch.equal(res.optimizer.master, full.optimizer.master)
    assert torch.equal(res.optimizer.exp_avg_sq, full.optimizer.exp_avg_sq)
    # save_merged: a transformers-loadable full model whose targets moved and whose other tensors did not
    full.save_merged(str(tmp_path / "merged"))
    msd = load_file(str(tmp_path / "merged" / "model.safetensors"))
    base = full.model.hf_state_dict()
    assert not torch.equal(msd["model.layers.0.self_attn.q_proj.weight"],
                           base["model.layers.0.self_attn.q_proj.weight"].cpu())
    assert torch.equal(msd["model.layers.0.self_attn.k_proj.weight"],
                       base["model.layers.0.self_attn.k_proj.weight"].cpu())
    assert torch.equal(msd["model.embed_tokens.weight"], base["model.embed_tokens.weight"].cpu())


def _dp_worker(rank, world, port, q, out_dir):
    """One fp32 LoRA GRPO step on this rank of two gloo ranks sharing the GPU."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), SWH_DIST_BACKEND="gloo")
    try:
        from swh_trl_amd.engine import CausalLM, LoraConfig, tiny_qwen2
        from swh_trl_amd.trainer import GRPOConfig, GRPOTrainer
        cfg = tiny_qwen2(512, 2)
        ds = [{"prompt": None, "prompt_ids": list(range(3 + 5 * i, 11 + 5 * i))} for i in range(32)]

        def rew(prompts=None, completions=None, completion_ids=None, **kw):
            return [float(len(set(c)) % 5) for c in completion_ids]

        args = GRPOConfig(per_device_train_batch_size=8, gradient_accumulation_steps=2, num_generations=4,
                          max_prompt_length=8, max_completion_length=16, max_steps=1, learning_rate=1e-3,
                          lr_scheduler_type="constant", shuffle_dataset=False,
                          generation_kwargs={"eos_token_id": 1, "pad_token_id": 0, "min_new_tokens": 4},
                          model_init_kwargs={"torch_dtype": "float32"}, logging_steps=1, seed=7)
        tr = GRPOTrainer(model=CausalLM(cfg, torch.device("cuda:0"), seed=3, init_std=0.05, dtype=torch.float32),
                         reward_funcs=rew, args=args, train_dataset=ds,
                         peft_config=LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"))
        _randomize_b(tr)  # B = 0 would leave dA = 0; the same values on both ranks
        base, a0 = _cpu(tr.model.hf_state_dict()), _cpu(tr.model.adapter_state_dict())
        cap = {}
        gen_fn = tr._generate_and_score_completions

        def gen_capture(examples):
            out = gen_fn(examples)
            cap["gen"] = {k: v.detach().cpu().clone() for k, v in out.items()}
            n = out["completion_ids"].shape[0]
            cap["perm"] = torch.randperm(n, generator=torch.Generator().set_state(tr._shuffle_gen.get_state()))
            return out

        tr._generate_and_score_completions = gen_capture
        tr.training_step_group()
        torch.cuda.synchronize()
        torch.save({"base": base, "a0": a0, "gen": cap["gen"], "perm": cap["perm"],
                    "grads": _cpu(tr.model.adapter_grad_state_dict()), "a1": _cpu(tr.model.adapter_state_dict())},
                   os.path.join(out_dir, f"rank{rank}.pt"))
        q.put((rank, "ok"))
    except Exception as e:  # surface the failure to the parent
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def test_dp_averaged_adapter_gradient_equals_mean_of_oracle_rank_gradients(tmp_path):
    from oracle import grpo_step as og
    from swh_trl_amd.engine import LoraConfig, lora, tiny_qwen2
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 1000)
    ps = [ctx.Process(target=_dp_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in ps:
        p.join(timeout=60)
    assert all(v == "ok" for v in got.values()), got
    runs = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(world)]
    for k in runs[0]["grads"]:
        assert torch.equal(runs[0]["grads"][k], runs[1]["grads"][k]), k  # one averaged gradient
        assert torch.equal(runs[0]["a1"][k], runs[1]["a1"][k]), k       # replicas stay identical
    assert not torch.equal(runs[0]["gen"]["completion_ids"], runs[1]["gen"]["completion_ids"])
    all_ids = torch.cat([r["gen"]["completion_ids"] for r in runs])

    def rew(cids, cmask):
        return [float(len(set(row[m.bool()].tolist())) % 5) for row, m in zip(cids, cmask)]

    cfg = tiny_qwen2(512, 2)
    spec = lora.resolve(LoraConfig(r=8, lora_alpha=16, target_modules="all-linear"))
    per_rank = []
    for r, run in enumerate(runs):
        hf = _oracle(cfg, run["base"], spec, run["a0"], torch.float32)
        opt = torch.optim.SGD([p for p in hf.parameters() if p.requires_grad], lr=0.0)
        g = {"prompt_ids": run["gen"]["prompt_ids"], "prompt_mask": run["gen"]["prompt_mask"].long(),
             "completion_ids": run["gen"]["completion_ids"], "perm": run["perm"], "world_completion_ids": all_ids,
             "rank": r}
        rec = og.grpo_train(hf, opt, [g], rew, num_generations=4, C=16, per_device_train_batch_size=8,
                            gradient_accumulation_steps=2, n_steps=1, eos_token_id=1, capture=True)[0]
        per_rank.append(_peft_named(rec["grads"].items()))
    assert set(per_rank[0]) == set(runs[0]["grads"])
    for k, mine in runs[0]["grads"].items():
        want = sum(p[k] for p in per_rank) / world
        rel = ((mine.float() - want).norm() / want.norm().clamp_min(1e-20)).item()
        assert rel <= 1e-3, (k, rel)  # the single-rank fp32 bound of _check_fp32
