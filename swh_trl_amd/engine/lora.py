"""LoRA adapters over a frozen Qwen2 / Llama decoder.

The reference trains one way only: `GRPOTrainer(peft_config=...)` wraps the
policy in a peft LoRA model (trl/trainer/grpo_trainer.py:653-699), drops the
reference copy because the adapter can be switched off (:853-856, :1886) and
merges the adapter into the weights for generation (:1335-1378).  This module
is that mode on the engine's flat buffers:

  * `LoraConfig` carries peft's field names; the trainer reads any object with
    these attributes (`resolve`), so a real `peft.LoraConfig` works where peft is
    installed.  Every field is implemented or accepted only at its no-op value.
  * `LoraCausalLM` is the frozen base `CausalLM` (no gradient buffer) plus ONE
    flat adapter buffer (model dtype) and ONE flat fp32 adapter-gradient buffer.
    For a target Linear W [N, K] the adapter is A [Rp, K] and Bt [Rp, N] (B stored
    transposed), Rp = r rounded up to 16 with zero pad rows (csrc/lora.hip).  The
    A matrices of the packed qkv (and gate/up) targets are stacked, so one
    lora_down serves the pack.
  * `adapters_disabled()` makes the model the base model (the reference pass of
    beta != 0); `decode_view()` hands the rollout engine merged bf16 weights.
"""
from __future__ import annotations

import contextlib
import math
import re
from dataclasses import dataclass, field
from typing import Any, Optional, Union

import torch
import torch.nn.functional as F

from .. import nn_ops
from .config import DecoderConfig
from .model import _ALIGN, CausalLM, _dw_stream, _main_gemm_fence, _OnStream, _tgemm_serves

TARGET_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
DEFAULT_TARGETS = ("q_proj", "v_proj")  # peft's TRANSFORMERS_MODELS_TO_LORA_TARGET_MODULES_MAPPING for qwen2 / llama
MAX_RANK = 64
_SUB = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
        "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
# packed projection of the engine -> the reference modules whose outputs it concatenates, in order
_PACKS = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",), "gu": ("gate_proj", "up_proj"),
          "down": ("down_proj",)}


@dataclass
class LoraConfig:
    """peft.LoraConfig's fields, as far as this engine reads them."""
    r: int = 8
    lora_alpha: float = 8
    target_modules: Optional[Union[list, str]] = None
    lora_dropout: float = 0.0
    bias: str = "none"
    use_rslora: bool = False
    use_dora: bool = False
    modules_to_save: Optional[list] = None
    task_type: Optional[str] = None
    init_lora_weights: Union[bool, str] = True
    rank_pattern: dict = field(default_factory=dict)
    alpha_pattern: dict = field(default_factory=dict)
    layers_to_transform: Optional[list] = None


@dataclass(frozen=True)
class LoraSpec:
    """A validated adapter configuration: what `resolve` makes of a config object."""
    r: int
    lora_alpha: float
    targets: tuple
    use_rslora: bool = False
    task_type: Optional[str] = None

    @property
    def scale(self) -> float:
        return scaling(self.r, self.lora_alpha, self.use_rslora)

    @property
    def rank_pad(self) -> int:
        return rank_pad(self.r)


def rank_pad(r: int) -> int:
    """Rows the rank-r adapter matrices are stored with (the MFMA tile height)."""
    return (int(r) + 15) // 16 * 16


def scaling(r: int, lora_alpha: float, use_rslora: bool = False) -> float:
    """peft's LoRA scale: lora_alpha / r, or lora_alpha / sqrt(r) with rsLoRA."""
    return float(lora_alpha) / (math.sqrt(r) if use_rslora else r)


def resolve_targets(target_modules, model_type: str = "qwen2") -> tuple:
    """target_modules -> the adapted modules in canonical order.  None is peft's
    default for qwen2 / llama (q_proj, v_proj); "all-linear" is every decoder-layer
    Linear (peft leaves the output layer out)."""
    if model_type not in ("qwen2", "llama"):
        raise ValueError(f"peft_config: LoRA is implemented for the qwen2 / llama decoders, not {model_type!r}")
    if target_modules is None:
        names = DEFAULT_TARGETS
    elif isinstance(target_modules, str):
        if target_modules != "all-linear":
            raise ValueError(f"peft_config.target_modules={target_modules!r}: a list of module names or "
                             "'all-linear' (regex targets are not supported)")
        names = TARGET_MODULES
    else:
        names = tuple(target_modules)
        bad = [n for n in names if n not in TARGET_MODULES]
        if bad or not names:
            raise ValueError(f"peft_config.target_modules: {bad or 'empty'} — expected names out of "
                             f"{', '.join(TARGET_MODULES)}")
    return tuple(n for n in TARGET_MODULES if n in names)


def resolve(cfg: Any, model_type: str = "qwen2") -> LoraSpec:
    """Validate a peft-style config object (read by attribute) into a LoraSpec.
    Nothing is silently ignored: a field this engine does not implement raises a
    ValueError naming it unless it holds its no-op value."""
    g = lambda k, d: getattr(cfg, k, d)  # noqa: E731
    r = g("r", 8)
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MAX_RANK:
        raise ValueError(f"peft_config.r={r!r}: an integer in 1..{MAX_RANK}")
    alpha = g("lora_alpha", 8)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not alpha > 0:
        raise ValueError(f"peft_config.lora_alpha={alpha!r}: a positive number")
    if g("lora_dropout", 0.0) != 0:
        raise ValueError("peft_config.lora_dropout must be 0 (the reference forces 0; dropout is not implemented)")
    if g("bias", "none") != "none":
        raise ValueError("peft_config.bias must be 'none' (trainable biases are not implemented)")
    if g("use_dora", False):
        raise ValueError("peft_config.use_dora must be False (DoRA is not implemented)")
    if g("modules_to_save", None):
        raise ValueError("peft_config.modules_to_save must be None (only the adapter matrices train)")
    for k in ("rank_pattern", "alpha_pattern", "layers_to_transform"):
        if g(k, None):
            raise ValueError(f"peft_config.{k} must be empty (one rank and alpha for every layer)")
    if g("init_lora_weights", True) is not True:
        raise ValueError("peft_config.init_lora_weights must be True (kaiming-uniform A, zero B)")
    task = g("task_type", None)
    task = getattr(task, "value", task)  # peft's TaskType enum
    if task not in (None, "CAUSAL_LM"):
        raise ValueError(f"peft_config.task_type={task!r}: None or CAUSAL_LM")
    tm = g("target_modules", None)
    if isinstance(tm, (set, frozenset)):  # peft stores a set
        tm = sorted(tm)
    return LoraSpec(r=r, lora_alpha=float(alpha), targets=resolve_targets(tm, model_type),
                    use_rslora=bool(g("use_rslora", False)), task_type=task)


def module_dims(cfg: DecoderConfig, module: str) -> tuple:
    """(in_features, out_features) of a reference Linear."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {"q_proj": (H, cfg.q_dim), "k_proj": (H, cfg.kv_dim), "v_proj": (H, cfg.kv_dim), "o_proj": (cfg.q_dim, H),
            "gate_proj": (H, I), "up_proj": (H, I), "down_proj": (I, H)}[module]


def _module_col0(cfg: DecoderConfig, module: str) -> int:
    """First output column of a module inside its packed projection."""
    return {"k_proj": cfg.q_dim, "v_proj": cfg.q_dim + cfg.kv_dim, "up_proj": cfg.intermediate_size}.get(module, 0)


def adapter_layout(cfg: DecoderConfig, spec: LoraSpec) -> tuple:
    """({name: (offset, shape)}, numel) of the flat adapter buffer.  Per layer i and
    packed projection P with adapted modules: `l{i}.P.A` [S Rp, K] (the S modules'
    A matrices stacked in pack order), then `l{i}.<module>.Bt` [Rp, N] each."""
    Rp = spec.rank_pad
    layout, off = {}, 0

    def add(name, *shape):
        nonlocal off
        layout[name] = (off, tuple(shape))
        off += (math.prod(shape) + _ALIGN - 1) // _ALIGN * _ALIGN

    for i in range(cfg.num_hidden_layers):
        for pack, modules in _PACKS.items():
            mods = [m for m in modules if m in spec.targets]
            if not mods:
                continue
            add(f"l{i}.{pack}.A", len(mods) * Rp, module_dims(cfg, mods[0])[0])
            for m in mods:
                add(f"l{i}.{m}.Bt", Rp, module_dims(cfg, m)[1])
    return layout, off


def peft_key(i: int, module: str, which: str) -> str:
    """peft's state-dict key of layer i's module: which = 'A' or 'B'."""
    return f"base_model.model.model.layers.{i}.{_SUB[module]}.{module}.lora_{which}.weight"


def _views(flat: torch.Tensor, layout: dict) -> dict:
    return {k: flat[o:o + math.prod(s)].view(s) for k, (o, s) in layout.items()}


def _a_rows(spec: LoraSpec, module: str) -> tuple:
    """(pack name, first row) of a module's A inside its pack's stacked A."""
    for pack, modules in _PACKS.items():
        if module in modules:
            mods = [m for m in modules if m in spec.targets]
            return pack, mods.index(module) * spec.rank_pad
    raise KeyError(module)


def unpack_adapter(flat: torch.Tensor, cfg: DecoderConfig, spec: LoraSpec) -> dict:
    """Flat buffer -> peft state dict: lora_A.weight [r, in], lora_B.weight [out, r]
    (unpadded, B transposed back).  Works on any device."""
    v = _views(flat, adapter_layout(cfg, spec)[0])
    out = {}
    for i in range(cfg.num_hidden_layers):
        for m in spec.targets:
            pack, r0 = _a_rows(spec, m)
            out[peft_key(i, m, "A")] = v[f"l{i}.{pack}.A"][r0:r0 + spec.r].clone()
            out[peft_key(i, m, "B")] = v[f"l{i}.{m}.Bt"][:spec.r].t().contiguous()
    return out


def pack_adapter(sd: dict, flat: torch.Tensor, cfg: DecoderConfig, spec: LoraSpec) -> None:
    """peft state dict -> flat buffer (pad rows zeroed).  Keys may carry peft's
    adapter name (`lora_A.default.weight`); the key set must be exactly the
    adapted modules'."""
    sd = {re.sub(r"\.lora_([AB])\.[^.]+\.weight$", r".lora_\1.weight", k): t for k, t in sd.items()}
    want = {peft_key(i, m, w) for i in range(cfg.num_hidden_layers) for m in spec.targets for w in "AB"}
    if set(sd) != want:
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        raise ValueError(f"adapter state dict does not match the adapted modules: missing {missing[:3]}, "
                         f"unexpected {extra[:3]}")
    v = _views(flat, adapter_layout(cfg, spec)[0])
    with torch.no_grad():
        flat.zero_()
        for i in range(cfg.num_hidden_layers):
            for m in spec.targets:
                kin, nout = module_dims(cfg, m)
                a, b = sd[peft_key(i, m, "A")], sd[peft_key(i, m, "B")]
                if tuple(a.shape) != (spec.r, kin) or tuple(b.shape) != (nout, spec.r):
                    raise ValueError(f"adapter tensors of layer {i} {m}: expected A {(spec.r, kin)}, B "
                                     f"{(nout, spec.r)}, got {tuple(a.shape)}, {tuple(b.shape)}")
                pack, r0 = _a_rows(spec, m)
                v[f"l{i}.{pack}.A"][r0:r0 + spec.r].copy_(a)
                v[f"l{i}.{m}.Bt"][:spec.r].copy_(b.t())


def adapter_config_dict(spec: LoraSpec, base_model_name_or_path: Optional[str] = None) -> dict:
    """adapter_config.json as peft writes its essentials."""
    return {"peft_type": "LORA", "r": spec.r, "lora_alpha": spec.lora_alpha, "target_modules": list(spec.targets),
            "lora_dropout": 0.0, "bias": "none", "use_rslora": spec.use_rslora, "use_dora": False,
            "task_type": spec.task_type or "CAUSAL_LM", "base_model_name_or_path": base_model_name_or_path,
            "fan_in_fan_out": False, "inference_mode": True, "init_lora_weights": True, "modules_to_save": None}


class _Slice:
    """One adapted module of a packed projection: its output columns, its Bt (and
    gradient) and its rows of the pack's stacked A."""
    __slots__ = ("col0", "n", "row0", "bt", "gbt")

    def __init__(self, col0, n, row0, bt, gbt):
        self.col0, self.n, self.row0, self.bt, self.gbt = col0, n, row0, bt, gbt


class _Adapted:
    """The adapter of one packed projection (what _LoraLinear needs)."""
    __slots__ = ("a", "ga", "slices", "r", "rp", "scale", "hip")

    def __init__(self, a, ga, slices, r, rp, scale, hip):
        self.a, self.ga, self.slices, self.r, self.rp, self.scale, self.hip = a, ga, slices, r, rp, scale, hip

    @property
    def one_call(self) -> bool:
        """The stacked A fits one kernel call (its pad rows are zero, so the stack is a rank-S Rp adapter)."""
        return self.a.shape[0] <= MAX_RANK


class _LoraLinear(torch.autograd.Function):
    """y = x W^T (+ b) + s (x A^T) B^T per adapted column slice, W and b frozen.

    Forward: the base GEMM exactly as `_Linear` routes it, then lora_down +
    lora_up_add per slice (u saved).  Backward: dx of the base GEMM as `_Linear`,
    v = lora_down(dy, Bt), dx += s v A, and the two adapter gradients accumulated
    into their fp32 views (swh_lora_grad: fixed-order chunks, no atomics).  With
    ad.hip False (an fp32 model, or EngineOptions.hip_lora False) the same math
    runs as a torch composition."""

    @staticmethod
    def forward(ctx, x, w, b, ad: _Adapted, opts):
        K, N = w.shape[1], w.shape[0]
        x2 = x.reshape(-1, K)
        y = None
        if _tgemm_serves(opts, N, K) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16:
            if nn_ops.gemm_nt_eligible(x2, w) and (b is None or b.dtype == torch.bfloat16):
                y = nn_ops.gemm_nt(x2, w, b)
        if y is None:
            y = F.linear(x2, w, b)
        if ad.hip:
            if not x2.is_contiguous():
                x2 = x2.contiguous()
            u = torch.empty(x2.shape[0], ad.a.shape[0], device=x.device, dtype=x.dtype)
            if ad.one_call:
                nn_ops.lora_down(x2, ad.a, ad.a.shape[0], out=u)
            for s in ad.slices:
                uj = u[:, s.row0:s.row0 + ad.rp]
                if not ad.one_call:
                    nn_ops.lora_down(x2, ad.a[s.row0:s.row0 + ad.rp], ad.r, out=uj)
                nn_ops.lora_up_add(y[:, s.col0:s.col0 + s.n], uj, s.bt, ad.r, ad.scale)
        else:
            u = x2 @ ad.a.t()
            for s in ad.slices:
                y[:, s.col0:s.col0 + s.n].addmm_(u[:, s.row0:s.row0 + ad.rp], s.bt, alpha=ad.scale)
        ctx.save_for_backward(x2, w, u)
        ctx.ad, ctx.opts, ctx.xshape = ad, opts, x.shape
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w, u = ctx.saved_tensors
        ad, opts = ctx.ad, ctx.opts
        N, K = w.shape
        dy2 = dy.reshape(-1, N)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            wt = None
            if _tgemm_serves(opts, N, K) and K % 128 == 0 and N % 64 == 0 and dy.dtype == torch.bfloat16 \
                    and w.dtype == torch.bfloat16:
                wt = w.t().contiguous()
            if wt is not None and nn_ops.gemm_nt_eligible(dy2, wt):
                dx = nn_ops.gemm_nt(dy2, wt)
            else:
                _main_gemm_fence(dy.device)
                dx = dy2 @ w
        v = torch.empty_like(u)
        if ad.hip:
            for s in ad.slices:
                nn_ops.lora_down(dy2[:, s.col0:s.col0 + s.n], s.bt, ad.r, out=v[:, s.row0:s.row0 + ad.rp])
            if dx is not None:  # dx += s v A on the compute stream (the next layer waits for it)
                if ad.one_call:
                    nn_ops.lora_up_add(dx, v, ad.a, ad.a.shape[0], ad.scale)
                else:
                    for s in ad.slices:
                        rows = slice(s.row0, s.row0 + ad.rp)
                        nn_ops.lora_up_add(dx, v[:, rows], ad.a[rows], ad.r, ad.scale)
            # the adapter gradients are leaves: beside the chain on the weight-gradient stream, as
            # _accumulate_dw (joined by dw_sync at the end of the backward)
            with _OnStream(_dw_stream(dy.device)) as side:
                side.keep(u, v, x2, dy2)
                if ad.one_call:
                    side.keep(nn_ops.lora_grad(ad.ga, v, x2, ad.a.shape[0], ad.scale))
                for s in ad.slices:
                    rows = slice(s.row0, s.row0 + ad.rp)
                    if not ad.one_call:
                        side.keep(nn_ops.lora_grad(ad.ga[rows], v[:, rows], x2, ad.r, ad.scale))
                    side.keep(nn_ops.lora_grad(s.gbt, u[:, rows], dy2[:, s.col0:s.col0 + s.n], ad.r, ad.scale))
        else:
            for s in ad.slices:
                rows = slice(s.row0, s.row0 + ad.rp)
                dys = dy2[:, s.col0:s.col0 + s.n]
                v[:, rows] = dys @ s.bt.t()
                s.gbt.addmm_(u[:, rows].t().float(), dys.float(), alpha=ad.scale)
            if dx is not None:
                dx.addmm_(v, ad.a, alpha=ad.scale)
            ad.ga.addmm_(v.t().float(), x2.float(), alpha=ad.scale)
        return (dx.view(ctx.xshape) if dx is not None else None), None, None, None, None


class _DecodeView(CausalLM):
    """The model as the rollout engine reads it (engine/decode.py: weights through
    `p` / `lm_weight()`, the prefill through `hidden_states`): a frozen CausalLM
    whose adapted matrices are the merged copies; every other tensor aliases the
    base buffer."""

    def __init__(self, model: "LoraCausalLM", merged: dict):  # no buffers of its own: super().__init__ is not run
        self.cfg, self.device, self.head, self.dtype = model.cfg, model.device, model.head, model.dtype
        self.options, self.layout, self.numel, self.flat = model.options, model.layout, model.numel, model.flat
        self.p = dict(model.p)
        self.p.update(merged)
        self.grad, self.g = None, {}
        self._anchor = model._anchor
        self._rope = None
        self.on_layer_grads = None


class LoraCausalLM(CausalLM):
    """The frozen base decoder (`flat`, no gradient buffer) + the adapter:
    `adapter` (flat, model dtype; views in `a`) and `adapter_grad` (flat fp32;
    views in `ga`).  Only the adapter trains; the embedding, norms and lm head
    stay frozen and dx still flows to layer 0."""

    def __init__(self, cfg: DecoderConfig, device, spec: LoraSpec, dtype=torch.bfloat16, seed: Optional[int] = 0,
                 adapter_seed: int = 0, init_std: float = 0.02, options=None):
        if cfg.model_type not in ("qwen2", "llama"):
            raise ValueError(f"LoRA is implemented for the qwen2 / llama decoders, not {cfg.model_type!r}")
        super().__init__(cfg, device, head="lm", dtype=dtype, seed=seed, init_std=init_std, trainable=False,
                         options=options)
        self.spec = spec
        self.adapter_layout, self.adapter_numel = adapter_layout(cfg, spec)
        self.adapter = torch.zeros(self.adapter_numel, device=self.device, dtype=dtype)
        self.adapter_grad = torch.zeros(self.adapter_numel, device=self.device, dtype=torch.float32)
        self.a = _views(self.adapter, self.adapter_layout)
        self.ga = _views(self.adapter_grad, self.adapter_layout)
        self._enabled = True
        self._merged: Optional[dict] = None
        self._merge_tabs: Optional[list] = None
        self._view: Optional[_DecodeView] = None
        self._adapted: dict = {}
        self.init_adapter(adapter_seed)

    # ------------------------------------------------------------------ adapter weights
    @property
    def _hip_lora(self) -> bool:
        """The adapter path on csrc/lora.hip (bf16); options.hip_lora False, or an fp32
        model (the reference-precision mode), runs the same math as a torch composition."""
        return self.dtype == torch.bfloat16 and self.options.hip_lora

    def init_adapter(self, seed: int) -> None:
        """peft's init: A ~ U(-1/sqrt(K), 1/sqrt(K)) (kaiming-uniform, a = sqrt(5)), B = 0;
        pad rows zero.  A device generator seeded from `seed` (the trainer's args.seed)."""
        g = torch.Generator(device=self.device).manual_seed(int(seed))
        r, Rp = self.spec.r, self.spec.rank_pad
        with torch.no_grad():
            self.adapter.zero_()
            for name, t in self.a.items():
                if not name.endswith(".A"):
                    continue
                bound = 1.0 / math.sqrt(t.shape[1])
                for r0 in range(0, t.shape[0], Rp):
                    t[r0:r0 + r].copy_((torch.rand(r, t.shape[1], generator=g, device=self.device,
                                                   dtype=torch.float32) * 2 - 1) * bound)

    def zero_grad(self):
        self.adapter_grad.zero_()

    def no_decay_ranges(self) -> list:
        """A and B are Linear weights: weight decay everywhere."""
        return []

    def adapter_state_dict(self) -> dict:
        return unpack_adapter(self.adapter, self.cfg, self.spec)

    def adapter_grad_state_dict(self) -> dict:
        """The adapter gradients under peft's names (fp32), shaped as the weights."""
        return unpack_adapter(self.adapter_grad, self.cfg, self.spec)

    def load_adapter_state_dict(self, sd: dict) -> None:
        pack_adapter({k: t.to(self.device) for k, t in sd.items()}, self.adapter, self.cfg, self.spec)

    @contextlib.contextmanager
    def adapters_disabled(self):
        """Inside, every forward is the base model's (bit for bit a plain CausalLM
        with these weights): the reference pass of beta != 0."""
        old, self._enabled = self._enabled, False
        try:
            yield self
        finally:
            self._enabled = old

    # ------------------------------------------------------------------ forward
    def _adapted_of(self, name: str) -> Optional[_Adapted]:
        """`l{i}.qkv_w` -> its _Adapted (None when no module of the pack is a target)."""
        if name in self._adapted:
            return self._adapted[name]
        layer, pack = name[:-2].split(".")
        mods = [m for m in _PACKS[pack] if m in self.spec.targets]
        ad = None
        if mods:
            Rp = self.spec.rank_pad
            slices = [_Slice(_module_col0(self.cfg, m), module_dims(self.cfg, m)[1], j * Rp,
                             self.a[f"{layer}.{m}.Bt"], self.ga[f"{layer}.{m}.Bt"]) for j, m in enumerate(mods)]
            ad = _Adapted(self.a[f"{layer}.{pack}.A"], self.ga[f"{layer}.{pack}.A"], slices, self.spec.r, Rp,
                          self.spec.scale, self._hip_lora)
        self._adapted[name] = ad
        return ad

    def _proj(self, name: str, x: torch.Tensor) -> torch.Tensor:
        ad = self._adapted_of(name) if self._enabled else None
        if ad is None:
            return super()._proj(name, x)
        ad.hip = self._hip_lora
        return _LoraLinear.apply(x, self.p[name], self.p.get(name[:-2] + "_b"), ad, self.options)

    # ------------------------------------------------------------------ merged weights
    def _merge_jobs(self):
        """(name of the packed weight, W rows, A rows, Bt, out rows) per adapted module."""
        Rp = self.spec.rank_pad
        for i in range(self.cfg.num_hidden_layers):
            for pack, modules in _PACKS.items():
                mods = [m for m in modules if m in self.spec.targets]
                for j, m in enumerate(mods):
                    c0, n = _module_col0(self.cfg, m), module_dims(self.cfg, m)[1]
                    yield (f"l{i}.{pack}_w", slice(c0, c0 + n), self.a[f"l{i}.{pack}.A"][j * Rp:(j + 1) * Rp],
                           self.a[f"l{i}.{m}.Bt"])

    @torch.no_grad()
    def merged_weights(self) -> dict:
        """{packed weight name: W + s B A rounded once to the model dtype} for every
        packed projection with an adapted module (buffers allocated once, refreshed
        on every call).  bf16: one swh_lora_merge launch per 256 jobs; rows of a
        pack that belong to no target are copied."""
        jobs = list(self._merge_jobs())
        if self._merged is None:
            self._merged = {name: torch.empty_like(self.p[name]) for name in {j[0] for j in jobs}}
        covered = {}
        for name, rows, _, _ in jobs:
            covered[name] = covered.get(name, 0) + (rows.stop - rows.start)
        for name, n in covered.items():
            if n != self.p[name].shape[0]:
                self._merged[name].copy_(self.p[name])
        if self._hip_lora:
            if self._merge_tabs is None:
                spec = [(self.p[n][rows], a, bt, self._merged[n][rows], self.spec.r, self.spec.scale)
                        for n, rows, a, bt in jobs]
                self._merge_tabs = [nn_ops.lora_merge_table(spec[k:k + nn_ops.LORA_MERGE_MAX_JOBS], self.device)
                                    for k in range(0, len(spec), nn_ops.LORA_MERGE_MAX_JOBS)]
            for tab in self._merge_tabs:
                nn_ops.lora_merge(*tab)
        else:
            for n, rows, a, bt in jobs:
                w = self.p[n][rows]
                self._merged[n][rows].copy_(torch.addmm(w.float(), bt.float().t(), a.float(), alpha=self.spec.scale))
        return self._merged

    def decode_view(self) -> _DecodeView:
        """The model as the rollout engine reads it, over the merged weights: re-merges
        on every call (once per generation) and returns the same view object."""
        merged = self.merged_weights()
        if self._view is None:
            self._view = _DecodeView(self, merged)
        return self._view

    @classmethod
    def from_base(cls, base: CausalLM, spec: LoraSpec, adapter_seed: int = 0) -> "LoraCausalLM":
        """A LoRA model over `base`'s weights (its flat buffer is adopted, not copied)."""
        if base.head != "lm":
            raise ValueError("LoRA adapts a causal LM (lm head)")
        m = cls(base.cfg, base.device, spec, dtype=base.dtype, seed=None, adapter_seed=adapter_seed,
                options=base.options)
        m.flat = base.flat
        m.p = {k: m.flat[o:o + math.prod(s)].view(s) for k, (o, s) in m.layout.items()}
        return m

    def merged_hf_state_dict(self) -> dict:
        """A transformers state dict of W + s B A (the merge in fp32, one rounding):
        the very weights the rollout engine decodes from."""
        p = dict(self.p)
        p.update({k: t.clone() for k, t in self.merged_weights().items()})
        old, self.p = self.p, p
        try:
            return self.hf_state_dict()
        finally:
            self.p = old
