"""Trained-like TextPoseTransformer weights for the stress tests (tests/test_tpt_stress_*.py and
tests/golden/make_golden_tpt_stress.py share them).  A helper module, not a conftest.py: the tests import it by name.

The suite's one weight recipe (tpt_train_ref.recipe_state: seeded default init + 0.05 noise) gives near-uniform softmax
rows, scores that span about one unit and LayerNorm rows of variance O(1).  The recipes here turn such a state into one
whose heads lock onto one or two keys (`peaked`), whose logits carry row-constant offsets of +-100 from the K bias
(`offset`) and whose final LayerNorms see rows of variance below or near eps (`lnvar`) -- deterministically, from the
weights alone.  Every recipe returns a new dict and leaves its argument (a shared, cached state) unchanged.

The bars of the stress tests are the project's own: y by the rule of tests/test_tenc_params.py (`y_bar`), gradients by
train_ref.assert_within_bar.  The caps CAP_Y32 and CAP_G32 keep those relative bars sharp: a case goes to the GPU only
if the float32 CPU port itself stays below them (asserted in test_tpt_stress_cpu.py)."""
import functools
import math

import torch

import tpt_ref
from tpt_train_ref import layer_counts, port_forward, recipe_state

N_TOKENS = 50
LAYERS = (2, 2)
FACTOR = 3.0                  # `peaked`: Q and K rows x3, the weight part of every logit x9
AMOUNT = 100.0                # `offset`: the row-constant logit offset of the two chosen heads
Q_ALONG = 8.0                 # `offset`: every query's component along the head's direction d
HEAD_POS, HEAD_NEG = 1, 2     # `offset`: the head that gets +AMOUNT and the one that gets -AMOUNT
K = {"fp32": 4.0, "f16x3": 16.0}   # tests/test_tenc_params.py: factors on the float32 port's own error
CAP_Y32 = 10 * tpt_ref.BAR    # condition (b): max|y32 - y64| of `peaked` and `offset` cases
CAP_G32 = 1e-3                # condition (b): per tensor max|g32 - g64| / max|g64| of training cases
MIN_ROW_MAX = 0.5             # condition (a): mean row-maximum probability in every attention of a case
MIN_OFFSET = 89.0             # condition (a): exp overflows in float32 beyond 88.7
NEG_LOGIT = -20.0             # condition (a): every real-key logit of the negative head lies below
SEED = 700                    # recipe_state seed of the stressed states


def attentions(state):
    """(trace key of port_forward, state_dict prefix, kind) of every attention of the model, in forward order."""
    n_enc, n_dec = layer_counts(state)
    out = [(("enc", l, "probs"), f"transformer.encoder.layers.{l}.self_attn.", "enc") for l in range(n_enc)]
    for l in range(n_dec):
        pre = f"transformer.decoder.layers.{l}."
        out += [(("dec", l, "self_probs"), pre + "self_attn.", "self"), (("dec", l, "cross_probs"), pre + "multihead_attn.", "cross")]
    return out


def _query_mean(state, prefix):
    """The mean row that enters the Q projection of attention `prefix`, from the weights: the bias of the LayerNorm
    in front of it, or of pose2hidden_projection, or the mean row of the embedding table."""
    pre, name = prefix.rsplit(".", 2)[0] + ".", prefix.rsplit(".", 2)[1]
    side, l = pre.split(".")[1], int(pre.split(".")[3])
    if name == "multihead_attn":
        return state[pre + "norm1.bias"].double()
    if l > 0:
        return state[f"transformer.{side}.layers.{l - 1}.norm{2 if side == 'encoder' else 3}.bias"].double()
    if side == "encoder":
        return state["token_embedding.weight"].double().mean(0)
    return state["pose2hidden_projection.bias"].double()


def dec0_factor(state, factor=FACTOR, pose_std=1.0):
    """The Q/K factor of layer 0's decoder self-attention.  Every other attention reads LayerNorm rows (variance ~1 per
    component); this one reads h = W x + b of pose2hidden_projection, un-normalised.  For zero-mean rows of covariance C
    the scores q.k / sqrt(32) of head h have variance tr(Wk_h C Wk_h' Wq_h C Wq_h') / 32; scaling Q and K by f scales
    the scores by f^2.  So f = factor * (var at C = I / var at C = pose_std^2 W W')^(1/4), averaged over the heads,
    makes this attention as peaked as `factor` makes the others -- from the weights alone, for poses of `pose_std`."""
    W = state["pose2hidden_projection.weight"].double()
    ipw = state["transformer.decoder.layers.0.self_attn.in_proj_weight"].double()

    def var(C):
        return sum(float(torch.trace(ipw[128 + 32 * h:160 + 32 * h] @ C @ ipw[128 + 32 * h:160 + 32 * h].T
                                     @ ipw[32 * h:32 * h + 32] @ C @ ipw[32 * h:32 * h + 32].T)) for h in range(4)) / 4
    return factor * (var(torch.eye(128, dtype=torch.float64)) / var(pose_std ** 2 * W @ W.T)) ** 0.25


def peaked(state, factor=FACTOR, pose_std=1.0):
    """Q and K rows (weight and bias) of in_proj of EVERY attention scaled by `factor`; layer 0's decoder
    self-attention by dec0_factor."""
    st = {k: v.clone() for k, v in state.items()}
    f0 = dec0_factor(state, factor, pose_std)
    for _, pre, _ in attentions(st):
        f = f0 if pre == "transformer.decoder.layers.0.self_attn." else factor
        st[pre + "in_proj_weight"][:256] *= f
        st[pre + "in_proj_bias"][:256] *= f
    return st


def offset(state, amount=AMOUNT, q_along=Q_ALONG):
    """In every attention, heads HEAD_POS and HEAD_NEG get logits that carry the row constant +amount and -amount.
    d = the head's mean query direction (Wq_h mu + bq_h, mu = _query_mean).  The Q rows lose their component along d
    and the Q bias gets q_along * d instead, so every query has q . d = q_along; the K bias gets
    +-amount * sqrt(32) / q_along * d.  Every score of the head then moves by +-amount, which softmax cancels in exact
    arithmetic -- and which overflows exp without the maximum subtraction, sits in the running maximum and the saved
    log-sum-exp of the blocked kernels, and in HEAD_NEG leaves every real key far below a padded key that reads as
    zeros (score 0) or as the K bias alone (score -amount, level with the real keys)."""
    st = {k: v.clone() for k, v in state.items()}
    for _, pre, _ in attentions(st):
        w, b = st[pre + "in_proj_weight"], st[pre + "in_proj_bias"]
        mu = _query_mean(state, pre)
        for h, sign in ((HEAD_POS, 1.0), (HEAD_NEG, -1.0)):
            q, k = slice(32 * h, 32 * h + 32), slice(128 + 32 * h, 160 + 32 * h)
            d = w[q].double() @ mu + b[q].double()
            d = d / d.norm()
            proj = torch.eye(32, dtype=torch.float64) - torch.outer(d, d)
            w[q] = (proj @ w[q].double()).float()
            b[q] = (proj @ b[q].double() + q_along * d).float()
            b[k] = (b[k].double() + sign * amount * math.sqrt(32.0) / q_along * d).float()
    return st


def lnvar(state, gamma=1e-3, beta=30.0, seed=SEED + 1, encoder=True):
    """The last decoder layer's norm3 and (`encoder`) the last encoder layer's norm2 get gain gamma * N(0, 1) and bias
    beta, so the stack norms behind them (transformer.decoder.norm, transformer.encoder.norm) see rows of mean beta and
    variance ~gamma^2: below eps = 1e-5 at gamma = 1e-3 (rstd ~ 1/sqrt(eps), and the rows' own float32 rounding, ulp
    1.9e-6 at 30, is amplified 300-fold).  The mild variant for training has variance about eps (gamma = 3e-3) and
    leaves the encoder alone: the memory rows would carry that amplified rounding (~1e-3) into every ReLU input of the
    decoder, where no draw can keep the ReLU margin (a ReLU input within 2e-3 of zero is a certainty among 1e4)."""
    st = {k: v.clone() for k, v in state.items()}
    n_enc, n_dec = layer_counts(st)
    g = torch.Generator().manual_seed(seed)
    for pre in ([f"transformer.encoder.layers.{n_enc - 1}.norm2."] if encoder else []) + [f"transformer.decoder.layers.{n_dec - 1}.norm3."]:
        st[pre + "weight"] = gamma * torch.randn((128,), generator=g)
        st[pre + "bias"] = torch.full((128,), float(beta))
    return st


LNVAR_MILD = 3e-3
RECIPES = {
    "peaked": lambda st: peaked(st),
    "offset": lambda st: offset(peaked(st)),
    "lnvar": lambda st: lnvar(st),
    "lnvar_mild": lambda st: lnvar(st, gamma=LNVAR_MILD, encoder=False),
}


@functools.lru_cache(maxsize=None)
def stressed_state(recipe, seed=SEED, n_tokens=N_TOKENS, layers=LAYERS):
    """RECIPES[recipe] on recipe_state(seed, n_tokens, *layers); cached and shared, so leave it unchanged."""
    return RECIPES[recipe](recipe_state(seed, n_tokens, *layers))


def stress_inputs(B, S, T, n_tokens, seed):
    """Distinct-looking tokens (no padding run: equal key rows would share a row's weight) and N(0, 1) poses, the
    scale dec0_factor assumes."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, n_tokens - 1, (B, S), generator=g), torch.randn((B, T, 12, 2), generator=g)


def ramp_pose(state, B, T, seed, rise=60.0, jitter=8.0, flat=()):
    """The pose ramp of test_row_maximum_in_a_later_key_block for `state`: x_t = v + (t / T) u + sigma * noise with a
    large constant v, so that every query of layer 0's decoder self-attention is close to q = Wq (W v + b) + bq.  u
    solves q_h . Wk_h W u / sqrt(32) = rise for every head, = 0 for the heads in `flat` (a 4 x 24 system, from the
    weights alone): the scores rise by `rise` from the first key to the last and the running maximum of a blocked
    kernel moves in every key block; with flat = (HEAD_NEG,) that head's real keys stay where `offset` put them, far
    below zero.  sigma is set so that the noise moves a key's score by `jitter` (rms over the heads): one key of the last stretch stands out and
    the rows are peaked, not merely slanted.  Every frame carries the same large v, so the rows that reach the LATER
    decoder layers are nearly equal and their self-attentions near-uniform: a ramp case names layer 0's only."""
    st = {k: v.double() for k, v in state.items()}
    g = torch.Generator().manual_seed(seed)
    v = 5.0 * torch.randn((24,), generator=g).double()
    W, b = st["pose2hidden_projection.weight"], st["pose2hidden_projection.bias"]
    ipw, ipb = (st["transformer.decoder.layers.0.self_attn.in_proj_" + n] for n in ("weight", "bias"))
    q = ipw[:128] @ (W @ v + b) + ipb[:128]
    G = torch.stack([W.T @ ipw[128 + 32 * h:160 + 32 * h].T @ q[32 * h:32 * h + 32] for h in range(4)]) / math.sqrt(32.0)
    want = torch.full((4,), float(rise), dtype=torch.float64)
    want[list(flat)] = 0.0
    u = torch.linalg.pinv(G) @ want
    sigma = jitter / float(G.norm(dim=1).pow(2).mean().sqrt())
    ramp = torch.arange(T, dtype=torch.float64).reshape(1, T, 1) / T
    x = v + ramp * u + sigma * torch.randn((B, T, 24), generator=g).double()
    return x.reshape(B, T, 12, 2).float()


def ports(tokens, pose, state):
    """(y64, y32, trace64) of port_forward without dropout: the float64 truth, the float32 port and the float64
    attention probabilities, memory and tgt rows."""
    trace = {}
    with torch.no_grad():
        y64 = port_forward(tokens, pose.double(), {k: v.double() for k, v in state.items()}, {}, 0.0, torch.float64, trace)
        y32 = port_forward(tokens, pose.float(), {k: v.float() for k, v in state.items()}, {}, 0.0, torch.float32)
    return y64, y32, trace


def y_bar(y64, y32, k, floor=True):
    """max(BAR * max(1, max|y64|), k * max|y32 - y64|); without the floor for the near-eps LayerNorm case."""
    err32 = float((y32.double() - y64).abs().max())
    return max(tpt_ref.BAR * max(1.0, float(y64.abs().max())) if floor else 0.0, k * err32)


def logits(tokens, pose, state):
    """The float64 scores (B, 4, Tq, Tk) of every attention on this input, in the order of `attentions`: the
    arguments of the float64 port's softmax calls."""
    seen = []
    soft = torch.softmax

    def watched(s, dim):
        seen.append(s.detach().clone())
        return soft(s, dim=dim)
    torch.softmax = watched
    try:
        with torch.no_grad():
            port_forward(tokens, pose.double(), {k: v.double() for k, v in state.items()}, {}, 0.0, torch.float64)
    finally:
        torch.softmax = soft
    assert len(seen) == len(attentions(state))
    return seen


def row_stats(tokens, pose, state):
    """Per attention, on the float64 port: the mean row-maximum probability, per head the smallest key index of a row
    maximum, and of heads HEAD_POS / HEAD_NEG the row offsets nearest to zero and the largest real-key logit of HEAD_NEG.
    The row offset is what the K bias adds to a row's scores: the scores minus those of the same state with every K
    bias zeroed (softmax cancels a K bias, so the rows that enter every later attention are the same to 1e-12); it
    must be the same for every key of a row."""
    _, _, trace = ports(tokens, pose, state)
    bare = {k: v.clone() for k, v in state.items()}
    for _, pre, _ in attentions(state):
        bare[pre + "in_proj_bias"][128:256] = 0
    out = {}
    for (key, pre, kind), s, s0 in zip(attentions(state), logits(tokens, pose, state), logits(tokens, pose, bare)):
        off = s - s0
        assert float((off - off[..., :1]).abs().max()) <= 1e-6 * max(1.0, float(off.abs().max())), key
        out[key] = dict(kind=kind, row_max=float(trace[key].max(-1).values.mean()),
                        argmax_min=[int(trace[key][:, h].argmax(-1).min()) for h in range(4)],
                        pos_offset=float(off[:, HEAD_POS].min()), neg_offset=float(off[:, HEAD_NEG].max()),
                        neg_top=float(s[:, HEAD_NEG].max()))
    return out


# ---- the cases of test_tpt_stress_gpu.py, and the conditions (a) and (b) that admit them --------------------------
KB = 128                                                # key block of the blocked kernels; the short-path limit
SHAPES = [(2, 17, 33), (3, 33, 128), (1, 17, 130), (1, 9, 2 * KB + 44)]
# (recipe, shape, pose kind): every state at every shape on N(0, 1) poses; beyond 128 frames `peaked` and `offset` on the
# ramp as well
INFER_CASES = [(r, s, "plain") for r in ("peaked", "offset", "lnvar") for s in SHAPES] + \
              [(r, s, "ramp") for r in ("peaked", "offset") for s in SHAPES[2:]]
# Training.  The ReLU-margin rule of test_tpt_train_long_gpu._check_case (no float64 ReLU input closer to zero than
# twice the float32 port's largest rounding of any) decides the geometry: under `peaked` / `offset` a second layer
# compounds the float32 port's rounding to 5e-5 .. 7e-4 and NO draw of 12 keeps the margin at any shape from 128 frames
# on (3 of 12 at (2, 17, 33)); with one layer each and one sequence it is 1e-5 .. 5e-5 and every second draw passes.
# `lnvar_mild` keeps 2 + 2 layers (rounding 3e-6, 11 draws of 12 pass).  On the ramp, dropout raises the rounding of
# the near-equal rows tenfold and again no draw of 12 passes: the ramp trains at p = 0 only, the N(0, 1) poses at
# both p (test_row_maximum_in_a_later_key_block has the ramp at p = 0.1 under the recipe weights).
TRAIN_LAYERS = {"peaked": (1, 1), "offset": (1, 1), "lnvar_mild": LAYERS}
TRAIN_SHAPES = [(2, 17, 33), (1, 33, 128), (1, 17, 130), (1, 9, 2 * KB + 44)]
# (recipe, shape, pose kind, train kernels, p)
TRAIN_CASES = [(r, s, kind, route, p)
               for r in TRAIN_LAYERS for s in TRAIN_SHAPES
               for kind in ["plain"] + (["ramp"] if s[2] > 2 * KB and r != "lnvar_mild" else [])
               for route in ["valu"] + (["mfma"] if s[2] > KB else [])
               for p in ([0.0, 0.1] if kind == "plain" else [0.0])]


def train_state(recipe):
    return stressed_state(recipe, layers=TRAIN_LAYERS[recipe])


def case_id(case):
    return "-".join("b%d_s%d_t%d" % c if isinstance(c, tuple) else str(c) for c in case)


def case_inputs(recipe, shape, kind, attempt=0, state=None):
    """(tokens, pose) of a case; `attempt` counts the draws of the ReLU-margin rule (test_tpt_train_long_gpu.py);
    `state`: the stressed state the ramp is derived from, where it is not stressed_state(recipe)."""
    B, S, T = shape
    seed = 7000 + 10 * S + T + 100000 * attempt
    tok, pose = stress_inputs(B, S, T, N_TOKENS, seed)
    if kind == "ramp":
        pose = ramp_pose(stressed_state(recipe) if state is None else state, B, T, seed + 1,
                         flat=(HEAD_NEG,) if recipe == "offset" else ())
    return tok, pose


def named(state, kind):
    """The attentions a case names for condition (a): all of them, or on the ramp all but the later decoder layers'
    self-attentions (see ramp_pose)."""
    return [key for key, _, _ in attentions(state) if not (kind == "ramp" and key[2] == "self_probs" and key[1] > 0)]


def check_inputs(recipe, kind, tokens, pose, y64, y32, state=None):
    """Conditions (a) and (b) of a `peaked` / `offset` case on the CPU ports; returns the figures."""
    state = stressed_state(recipe) if state is None else state
    err32 = float((y32.double() - y64).abs().max())
    stats = row_stats(tokens, pose, state) if recipe in ("peaked", "offset") else {}
    if not stats:
        return err32, stats
    assert err32 <= CAP_Y32, f"{recipe} {kind}: the float32 port is {err32:.2e} off"
    for key in named(state, kind):
        v = stats[key]
        assert v["row_max"] >= MIN_ROW_MAX, (recipe, kind, key, v)
        if recipe == "offset":
            assert v["pos_offset"] > MIN_OFFSET and v["neg_offset"] < -MIN_OFFSET and v["neg_top"] <= NEG_LOGIT, (key, v)
    if kind == "ramp" and pose.shape[1] > 2 * KB:       # every row's maximum lies behind the first key block
        first = stats[("dec", 0, "self_probs")]["argmax_min"]
        assert all(first[h] >= KB for h in range(4) if not (recipe == "offset" and h == HEAD_NEG)), first
    return err32, stats


def check_gradients(names, g64, g32):
    """Condition (b) for training: per tensor max|g32 - g64| <= CAP_G32 * max|g64|; returns the worst ratio."""
    worst = (0.0, "")
    for k, a, b in zip(names, g64, g32):
        a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
        rel = float((b - a).abs().max() / a.abs().max())
        worst = max(worst, (rel, k))
    assert worst[0] <= CAP_G32, f"the float32 port's gradient of {worst[1]} is {worst[0]:.2e} (relative) off"
    return worst


def admit(recipe, kind):
    """The `admit` of test_tpt_train_long_gpu._check_case for a training case: conditions (a) and (b) on the CPU ports."""
    from tpt_train_ref import param_keys
    state = train_state(recipe)

    def refused(tokens, x, y64, y32, g64, g32):
        try:
            check_inputs(recipe, kind, tokens, x, y64, y32, state)
            check_gradients(param_keys(*TRAIN_LAYERS[recipe]) + ["dx"], g64, g32)
        except AssertionError as e:
            return str(e)
        return None
    return refused


def train_y_bar(y64, y32):
    return y_bar(y64, y32, K["fp32"])


# ---- the arithmetic of the training kernels, emulated on the port ------------------------------------------------
class SoftmaxRecomputed(torch.autograd.Function):
    """softmax whose backward recomputes P = exp(s - LSE) / sigma, sigma = rowsum(exp(s - LSE)), from a log-sum-exp
    saved in the scores' own precision, as all three training attentions do (b2h_tt_sdpa, b2h_lt_*, b2h_mt_*).
    `defect`: the saved LSE rounded to bfloat16's 8 significant bits and no division by sigma, which would forgive
    it -- what a kernel that saved its LSE too coarsely and trusted it would compute (the tests must see it)."""

    @staticmethod
    def forward(ctx, s, defect):
        lse = torch.logsumexp(s, -1, keepdim=True)
        ctx.defect = defect
        ctx.save_for_backward(s, lse.bfloat16().to(s.dtype) if defect else lse)
        return torch.exp(s - lse)

    @staticmethod
    def backward(ctx, dp):
        s, lse = ctx.saved_tensors
        p = torch.exp(s - lse)
        if not ctx.defect:
            p = p / p.sum(-1, keepdim=True)
        return p * (dp - (p * dp).sum(-1, keepdim=True)), None


def chain_matmul(a, b):
    """a @ b with ONE accumulator per output element: a fused multiply-add per term of the contraction, in ascending
    order, as the training attentions' threads sum (over d for a score, over the keys for O and dQ, over ALL queries of
    a sequence for dK and dV).  A float32 product is exact in float64, so rounding product + sum once is the fma."""
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=a.dtype)
    for t in range(a.shape[-1]):
        acc = (a[..., :, t, None].double() * b[..., t, None, :].double() + acc.double()).to(a.dtype)
    return acc


class MatmulByChain(torch.autograd.Function):
    """chain_matmul with chain_matmul gradients."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return chain_matmul(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        return chain_matmul(dc, b.transpose(-1, -2)), chain_matmul(a.transpose(-1, -2), dc)


class LinearByChain(torch.autograd.Function):
    """x W' + b as b2h_tt_linear forms it: the accumulator starts at the bias and takes one fused multiply-add per k,
    in ascending k.  torch adds the bias to the finished sum; where `offset` puts a K bias of 12 a component, every
    one of the 128 steps here rounds at that size instead of the one last step.  The gradients are torch's."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        acc = b.expand(x.shape[:-1] + (w.shape[0],)).clone()
        for k in range(w.shape[1]):
            acc = (x[..., k, None].double() * w[:, k].double() + acc.double()).to(x.dtype)
        return acc

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return dy @ w, dy.reshape(-1, dy.shape[-1]).T @ x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1]).sum(0)


def _attention_like_kernels(defect):
    import torch.nn.functional as F
    from tpt_train_ref import _drop

    def attention(xq, xkv, w, b, wo, bo, keep, p, trace, key):
        B, Tq, Tk = xq.shape[0], xq.shape[1], xkv.shape[1]
        q = F.linear(xq, w[:128], b[:128]).reshape(B, Tq, 4, 32).transpose(1, 2)
        k, v = (t.reshape(B, Tk, 4, 32).transpose(1, 2) for t in F.linear(xkv, w[128:], b[128:]).split(128, dim=-1))
        scores = MatmulByChain.apply(q, k.transpose(-1, -2)) * torch.tensor(1.0 / math.sqrt(32.0), dtype=q.dtype)   # the scale after the dot
        pd = _drop(SoftmaxRecomputed.apply(scores, defect), keep, p)
        return F.linear(MatmulByChain.apply(pd, v).transpose(1, 2).reshape(B, Tq, 128), wo, bo)
    return attention


def port_grads_like_kernels(tokens, pose, state, masks, p, dy, dtype, defect=False):
    """tpt_train_ref.port_grads in the arithmetic of the training kernels: the four products of an attention by
    MatmulByChain (the scale applied after the dot product), every softmax by SoftmaxRecomputed and every linear layer
    by LinearByChain.  In float64 it equals the plain port (1e-9); in float32 it is a second float32 implementation
    of the same mathematics.  Under `offset` the two differ from float64 by amounts that differ from each other
    several-fold in single tensors (test_tpt_stress_cpu.py measures it: this one is 2.4 - 3.3x further off in its
    worst tensor on every draw, mostly through LinearByChain), which leaves a bar of 4x ONE implementation's error no
    room for a draw on which that implementation happens to be close.  So the gradient bars of the `offset` training cases take the
    larger of the two ports' errors as a tensor's err32."""
    import torch.nn.functional as F
    import tpt_train_ref
    plain, linear = tpt_train_ref._attention, F.linear
    tpt_train_ref._attention = _attention_like_kernels(defect)
    F.linear = LinearByChain.apply
    try:
        return tpt_train_ref.port_grads(tokens, pose, state, masks, p, dy, dtype)
    finally:
        tpt_train_ref._attention, F.linear = plain, linear
