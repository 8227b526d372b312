"""The LoRA kernels (csrc/lora.hip) against the torch composition of the same
math at the bench micro-batch, and the LoRA GRPO step (measurement aid, not part
of the product).

    python tools/bench_lora.py [--tokens 6144] [--rank 16] [--reps 50] [--json OUT]
    python tools/bench_lora.py --step [--steps 10] [--warmup 3] [--runs 3] [--json OUT]

Kernel mode: T = 16 x 384 tokens, the Qwen2.5-0.5B projection shapes, r = 16.
Each row times one kernel and its torch composition on the same operands with
device events (warm-up first) and reports the bytes the operation has to move
(operands read once, result written once; up_add reads and writes its window)
over the time.  The torch compositions: F.linear (down), addmm_ into the column
window (up_add), a bf16 GEMM added into the fp32 gradient (grad), a per-matrix
fp32 addmm rounded to bf16 (merge).

Step mode: the bench step (64 x (128 + 256), micro-batch 16 x GA 4, beta 0) with
LoraConfig(r, 2 r, "all-linear"), `--runs` times in one process set-up each, and
the same loop without peft_config (full fine-tuning) beside it, alternating.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _t(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1000 * e0.elapsed_time(e1) / reps  # us


def kernels(a) -> list:
    import torch.nn.functional as F

    from swh_trl_amd import _lib, gemm_tuning, nn_ops
    from swh_trl_amd.engine import LoraCausalLM, LoraConfig, lora, qwen2_5_0_5b
    _lib.load()
    gemm_tuning.enable()
    cfg = qwen2_5_0_5b()
    T, r, s = a.tokens, a.rank, 2.0
    Rp = nn_ops.lora_rank_pad(r)
    H, I = cfg.hidden_size, cfg.intermediate_size
    bf = dict(device="cuda", dtype=torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)

    def rank(rows, cols, scale):
        m = rnd(rows, cols, scale=scale)
        for r0 in range(0, rows, Rp):
            m[r0 + r:r0 + Rp] = 0
        return m

    rows = []

    def row(name, t_hip, t_torch, nbytes):
        rec = {"op": name, "hip_us": round(t_hip, 1), "torch_us": round(t_torch, 1),
               "bytes": int(nbytes), "hip_GBps": round(nbytes / t_hip / 1e3, 1),
               "torch_GBps": round(nbytes / t_torch / 1e3, 1)}
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    # lora_down: u = x A^T on the hidden state (qkv stack of 3, gate/up stack of 2) and on the MLP activation
    for name, K, S in (("down x[T,896] qkv stack", H, 3), ("down x[T,896] gate/up stack", H, 2),
                       ("down a[T,4864] down_proj", I, 1), ("down dy[T,4864] (v = dy B, gate)", I, 1)):
        x, A = rnd(T, K), rank(S * Rp, K, K ** -0.5)
        u = torch.empty(T, S * Rp, **bf)
        row(name, _t(lambda: nn_ops.lora_down(x, A, S * Rp, out=u), a.reps), _t(lambda: F.linear(x, A), a.reps),
            2 * (T * K + S * Rp * K + T * S * Rp))
    # lora_up_add: y[:, window] += s u Bt
    for name, N, c0, C in (("up_add q of qkv", cfg.qkv_dim, 0, cfg.q_dim), ("up_add v of qkv", cfg.qkv_dim,
                                                                              cfg.q_dim + cfg.kv_dim, cfg.kv_dim),
                           ("up_add o / down", H, 0, H), ("up_add gate of gate/up", 2 * I, 0, I),
                           ("up_add up of gate/up", 2 * I, I, I), ("up_add dx[T,4864] (down dgrad)", I, 0, I)):
        y, u, Bt = rnd(T, N), rank(Rp, T, 1.0).t().contiguous(), rank(Rp, C, 0.02)
        win = y[:, c0:c0 + C]
        row(name, _t(lambda: nn_ops.lora_up_add(win, u, Bt, r, s), a.reps),
            _t(lambda: win.addmm_(u, Bt, alpha=s), a.reps), 2 * (2 * T * C + T * Rp + Rp * C))
    # lora_grad: G += s u^T in
    for name, C in (("grad dA / dBt over [T,896]", H), ("grad dBt q window [T,896] of qkv", -1),
                    ("grad over [T,4864]", I)):
        if C < 0:
            full = rnd(T, cfg.qkv_dim)
            x, C = full[:, :cfg.q_dim], cfg.q_dim
        else:
            x = rnd(T, C)
        u = rank(Rp, T, 1.0).t().contiguous()
        G = torch.zeros(Rp, C, device="cuda")
        row(name, _t(lambda: nn_ops.lora_grad(G, u, x, r, s), a.reps),
            _t(lambda: G.add_(u.t() @ x, alpha=s), a.reps), 2 * (T * C + T * Rp) + 8 * Rp * C)
    # lora_merge: every target of the 24-layer model, one launch
    spec = lora.resolve(LoraConfig(r=r, lora_alpha=2 * r, target_modules="all-linear"))
    m = LoraCausalLM(cfg, torch.device("cuda"), spec, seed=0)
    for k, t in m.a.items():
        if k.endswith(".Bt"):
            t[:r].copy_(rnd(r, t.shape[1], scale=0.02))
    nb = sum(2 * 2 * w.numel() for w in m.merged_weights().values()) + 2 * m.adapter_numel
    t_hip = _t(m.merged_weights, max(3, a.reps // 10))
    m.options = m.options.replace(hip_lora=False)
    t_torch = _t(m.merged_weights, max(3, a.reps // 10))
    row(f"merge {len(list(m._merge_jobs()))} matrices", t_hip, t_torch, nb)
    return rows


def _step_run(peft, a) -> dict:
    sys.path.insert(0, ROOT)
    import bench
    from swh_trl_amd.engine import LoraConfig
    from swh_trl_amd.engine.config import qwen2_5_0_5b
    from swh_trl_amd.trainer import GRPOConfig, GRPOTrainer
    cfg = qwen2_5_0_5b()
    if a.layers:
        cfg.num_hidden_layers = a.layers
    steps, warm = a.steps, a.warmup
    ds = bench.make_dataset(bench.PROMPTS_PER_GPU * (steps + warm + 1), cfg.vocab_size)
    gc = GRPOConfig(output_dir=None, per_device_train_batch_size=bench.MB, gradient_accumulation_steps=bench.GA,
                    num_generations=bench.G, max_prompt_length=bench.P, max_completion_length=bench.C,
                    learning_rate=1e-6, beta=a.beta, temperature=1.0, max_steps=steps + warm, logging_steps=10 ** 9,
                    seed=0, shuffle_dataset=True,
                    generation_kwargs={"min_new_tokens": bench.C, "eos_token_id": bench.EOS, "pad_token_id": bench.PAD})
    pc = LoraConfig(r=a.rank, lora_alpha=2 * a.rank, target_modules="all-linear") if peft else None
    tr = GRPOTrainer(model=cfg, reward_funcs=bench.dummy_reward, args=gc, train_dataset=ds, peft_config=pc)
    tr.state.max_steps = steps + warm
    for _ in range(warm):
        tr.training_step_group()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.training_step_group()
    torch.cuda.synchronize()
    ms = 1000 * (time.perf_counter() - t0) / steps
    del tr
    torch.cuda.empty_cache()
    return {"mode": "lora" if peft else "full", "ms_per_step": round(ms, 2), "samples_per_s": round(64e3 / ms, 2),
            "steps": steps, "warmup": warm, "beta": a.beta}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=6144)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--layers", type=int, default=None, help="debug only: shrink the model")
    ap.add_argument("--json", default=None, help="also write the records to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py measures on the GPU (no CPU fallback)")
    if a.step:
        out = []
        for _ in range(a.runs):
            for peft in (True, False):
                rec = _step_run(peft, a)
                print(json.dumps(rec), flush=True)
                out.append(rec)
    else:
        out = kernels(a)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
