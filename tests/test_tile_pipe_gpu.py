"""Launch policy tile_pipe: the tile kernel's pipelined prologue (a wave's first
tile runs the MFMAs of k-steps 0-15 under the landing of the rest of the X
image, behind hand-counted waits) against the load-all-then-compute prologue.
Same k order, same MFMAs, same epilogues: every output is bit-identical."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from swh_trl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _chunk_ss(t):
    M, H = t.shape
    return t.float().view(M, H // 16, 16).pow(2).sum(-1)


def _both(launch_policy, fn):
    """fn() under tile_pipe 1 and 0 (the tile kernel forced, to reach it at small N)."""
    outs = []
    for flag in (1, 0):
        launch_policy(gemm_tile=1, tile_pipe=flag)
        outs.append(fn())
    torch.cuda.synchronize()
    return outs


def test_tile_pipe_policy_field(dev, launch_policy):
    """The field is the last of the policy, 0 or 1, off by default or on as the library says."""
    from swh_trl_amd import _lib
    assert _lib.LaunchPolicy._fields_[-1][0] == "tile_pipe"
    assert _lib.get_launch_policy()["tile_pipe"] in (0, 1)
    launch_policy(tile_pipe=1)
    assert _lib.get_launch_policy()["tile_pipe"] == 1
    for bad in (-1, 2):
        with pytest.raises(Exception):
            _lib.set_launch_policy(tile_pipe=bad)
        assert _lib.get_launch_policy()["tile_pipe"] == 1


# M 37: clamped rows; M 16: one row group; N 128 / 256 leave most workgroups' waves without a
# tile (every wave still meets every barrier); N 4864: the bench's 608 tiles, waves with 0 and
# 1 tile in one workgroup; K 1024: the second compile-time K; K 512: not pipelined (falls back)
@pytest.mark.parametrize("M,N,K", [(64, 256, 896), (37, 256, 896), (16, 128, 896), (64, 256, 1024),
                                   (64, 4864, 896), (64, 256, 512)])
def test_tile_pipe_silu_gate_up(dev, launch_policy, M, N, K):
    from swh_trl_amd import nn_ops
    g = _gen(71)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(2 * N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev)
    wp = nn_ops.frag_pack(w, nw, silu=True)
    ss = _chunk_ss(x)
    acts = (0, 1) if M % 16 == 0 else (0,)  # the fragment-order output takes whole 16-row groups

    def run():
        return [nn_ops.decode_gemm_fragw(x, wp, eps=1e-6, silu=True, ss_in=ss, act_frag=a) for a in acts]

    on, off = _both(launch_policy, run)
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    if (M, N, K) == (64, 4864, 896):  # and against the fp32 product (test_decode_gemm_folded_norm's bounds)
        xf = x.float()
        xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).to(torch.bfloat16)).float()
        gu = (xn @ w.float().t()).to(torch.bfloat16)
        ref = (torch.nn.functional.silu(gu[:, :N]) * gu[:, N:]).float()
        torch.testing.assert_close(on[0].float(), ref, rtol=2e-2, atol=3e-2)


@pytest.mark.parametrize("M", [64, 37])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("fold", [False, True])
def test_tile_pipe_plain_and_bias(dev, launch_policy, M, bias, fold):
    """Plain / bias epilogues at N 512, K 896, row-major weights: plain X (no row scale)
    and the folded norm (row scale in the epilogue)."""
    from swh_trl_amd import nn_ops
    g = _gen(73)
    N, K = 512, 896
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    b = (0.1 * torch.randn(N, generator=g)).to(torch.bfloat16).to(dev) if bias else None
    ss = _chunk_ss(x) if fold else None
    on, off = _both(launch_policy, lambda: nn_ops.decode_gemm(x, w, eps=1e-6, bias=b, ss_in=ss))
    assert torch.equal(on, off)
    ref = x.float() @ w.float().t()
    if fold:
        ref = ref * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    if bias:
        ref = ref + b.float()
    torch.testing.assert_close(on.float(), ref, rtol=2e-2, atol=3e-2)


@pytest.mark.parametrize("kw", [dict(greedy=True), dict(), dict(temperature=0.7, min_new_tokens=5)])
def test_tile_pipe_leaves_the_fused_sampler_unchanged(dev, launch_policy, kw):
    """The pipelined prologue is restricted to the GEMM epilogues (SAMPLE 0): the fused
    lm-head sampler (V 40,000: some waves own two tiles) draws the same ids and writes
    the same log-probs, bit for bit, under either value of the field."""
    from swh_trl_amd import nn_ops, ops
    g = _gen(79)
    M, V, K = 64, 40000, 896
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(V, K, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    w[3] += 0.2
    ss = _chunk_ss(x)
    params = ops.make_sample_params(eos_token_ids=[3, 77], pad_token_id=5, **kw)
    rng = torch.tensor([123, 45], dtype=torch.int64, device=dev)
    stp = torch.tensor([2], dtype=torch.int32, device=dev)

    def run():
        res = []
        for logp in (False, True):
            out = torch.full((M, 4), -1, dtype=torch.int64, device=dev)
            cur = torch.empty(M, dtype=torch.int64, device=dev)
            fin = (torch.arange(M) % 7 == 0).int().to(dev)
            lp = torch.zeros(M, 4, dtype=torch.float32, device=dev) if logp else None
            nn_ops.lm_head_sample(x, w, params, rng, stp, fin, out, cur, eps=1e-6, ss_in=ss, out_logp=lp)
            res += [out, cur, fin] + ([lp] if logp else [])
        return res

    outs = []
    for flag in (1, 0):
        launch_policy(tile_pipe=flag)
        outs.append(run())
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_tile_pipe_generates_identically(dev, launch_policy):
    """A 2-layer Qwen2.5-0.5B-width engine, 16 rows x 12 new tokens: the same tokens and
    log-probs with the field 0 and 1, greedy and sampled."""
    from swh_trl_amd.engine import CausalLM, DecodeEngine
    from swh_trl_amd.engine.config import DecoderConfig
    m = CausalLM(DecoderConfig(num_hidden_layers=2), dev, seed=7, init_std=0.02)
    B, P, C = 16, 8, 12
    ids = torch.randint(0, m.cfg.vocab_size, (B, P), generator=_gen(17)).to(dev)
    mask = torch.ones(B, P, dtype=torch.int64, device=dev)
    outs = {}
    for flag in (1, 0):
        launch_policy(tile_pipe=flag)
        eng = DecodeEngine(m, B, P, C)
        outs[flag] = (eng.generate(ids, mask, C, greedy=True, return_logp=True),
                      eng.generate(ids, mask, C, temperature=0.9, seed=5, return_logp=True))
        del eng
    for a, b in zip(outs[1], outs[0]):
        for x, y in zip(a, b):
            if isinstance(x, torch.Tensor):
                assert torch.equal(x, y)
