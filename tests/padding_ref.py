"""Helpers of the key-padding-mask tests (tests/test_padding_*.py).  A helper module, not a conftest.py: the tests
import it by name.

The oracle is torch's own nn.Transformer on the CPU in float64 with src / tgt / memory key-padding masks
(`oracle_forward`), wrapped as the reference's TextPoseTransformer.forward wraps it (token_embedding, the two
projections) and loaded from the model's state_dict: the reference's class cannot take masks, so there are no golden
fixtures.  For dropout, `port_forward_masked` restates that forward with the keep-masks as inputs, in the manner of
tpt_train_ref.port_forward and from its pieces; tests/test_padding_masks_cpu.py pins it against the oracle at p = 0.

Lengths follow the product's rule: kl = clamp(length, 1, rows), key j attended iff j < kl.  Model outputs are compared
at frames < frame_lengths[b] only (`valid_frames`)."""
import functools
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from tpt_train_ref import _drop, layer_counts, leaf_state, param_keys, recipe_state

N_TOKENS = 50
BAR_Y = 2e-5      # max|y - y64| at valid frames: the project's fp32 transformer bar

# (B, S, T), text_lengths, frame_lengths, (n_enc, n_dec): the smallest shapes that reach every branch
WHOLE = ((3, 9, 17), (9, 4, 1), (17, 16, 5), (1, 1))            # full, one key, a 16-row tile boundary, a ragged tile
BLOCKED = ((4, 9, 200), (9, 4, 1, 7), (200, 129, 128, 70), (1, 1))   # full, one key into block 2, one block, block 2 skipped
DEEP = ((2, 40, 100), (40, 13), (100, 37), (2, 2))              # dMEM sums over decoder layers with masked rows
CASES = {"whole": WHOLE, "blocked": BLOCKED, "deep": DEEP}


def clamp_lengths(lengths, rows):
    return [min(max(int(n), 1), rows) for n in lengths]


def pad_mask(lengths, rows):
    """torch's key_padding_mask (B, rows): True = not attended."""
    return torch.arange(rows)[None, :] >= torch.tensor(clamp_lengths(lengths, rows))[:, None]


def valid_frames(frame_lengths, T):
    """(B, T) bool: the frames whose outputs are compared."""
    return ~pad_mask(frame_lengths, T)


def token_lengths_ref(tokens, pad_id=0):
    """numpy reference of hand_pose_sl_amd.token_lengths."""
    tok = np.asarray(tokens)
    out = np.ones(tok.shape[0], dtype=np.int64)
    for b in range(tok.shape[0]):
        keep = np.nonzero(tok[b] != pad_id)[0]
        if keep.size:
            out[b] = keep[-1] + 1
    return out


def oracle_forward(tokens, pose, state, text_lengths, frame_lengths, dtype=torch.float64):
    """nn.Transformer (post-norm, ReLU, p = 0, training mode so that no fused inference path is taken) with the three
    key-padding masks, between the reference's embedding and projections; `state` values of `dtype`."""
    n_enc, n_dec = layer_counts(state)
    B, T = pose.shape[0], pose.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        tr = torch.nn.Transformer(128, 4, n_enc, n_dec, 128, dropout=0.0, batch_first=True).to(dtype).train()
    # the state's own tensors stand in for the module's parameters, so that autograd reaches leaves among them
    weights = {k[len("transformer."):]: v for k, v in state.items() if k.startswith("transformer.")}
    assert set(weights) == set(dict(tr.named_parameters()))
    src = F.embedding(torch.as_tensor(tokens).long(), state["token_embedding.weight"])
    tgt = F.linear(pose.reshape(B, T, 24).to(dtype), state["pose2hidden_projection.weight"], state["pose2hidden_projection.bias"])
    ms = None if text_lengths is None else pad_mask(text_lengths, src.shape[1])
    mt = None if frame_lengths is None else pad_mask(frame_lengths, T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        h = torch.func.functional_call(tr, weights, (src, tgt), dict(src_key_padding_mask=ms, tgt_key_padding_mask=mt,
                                                                     memory_key_padding_mask=ms))
    y = F.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    return y.reshape(B, T, 21, 2)


def _attention(xq, xkv, w, b, wo, bo, keep, p, klen):
    """tpt_train_ref._attention with a key length per sequence: scores of keys >= kl are -inf before the softmax."""
    B, Tq, Tk = xq.shape[0], xq.shape[1], xkv.shape[1]
    q = F.linear(xq, w[:128], b[:128]).reshape(B, Tq, 4, 32).transpose(1, 2)
    k, v = (t.reshape(B, Tk, 4, 32).transpose(1, 2) for t in F.linear(xkv, w[128:], b[128:]).split(128, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(32.0)
    if klen is not None:
        s = s.masked_fill(pad_mask(klen, Tk)[:, None, None, :], float("-inf"))
    pd = _drop(torch.softmax(s, dim=-1), keep, p)
    return F.linear((pd @ v).transpose(1, 2).reshape(B, Tq, 128), wo, bo)


def port_forward_masked(tokens, pose, state, masks, p, dtype, text_lengths=None, frame_lengths=None):
    """tpt_train_ref.port_forward with the three key-padding masks: the encoder's self-attention and the decoder's
    cross-attention over `text_lengths`, the decoder's self-attention over `frame_lengths`."""
    B, T = pose.shape[0], pose.shape[1]
    n_enc, n_dec = layer_counts(state)

    def ln(h, pre):
        return F.layer_norm(h, (128,), state[pre + ".weight"], state[pre + ".bias"], 1e-5)

    def ff(h, pre, keep):
        f = _drop(F.relu(F.linear(h, state[pre + "linear1.weight"], state[pre + "linear1.bias"])), keep, p)
        return F.linear(f, state[pre + "linear2.weight"], state[pre + "linear2.bias"])

    def attn(xq, xkv, pre, keep, klen):
        return _attention(xq, xkv, state[pre + "in_proj_weight"], state[pre + "in_proj_bias"], state[pre + "out_proj.weight"],
                          state[pre + "out_proj.bias"], keep, p, klen)

    mem = F.embedding(torch.as_tensor(tokens).long(), state["token_embedding.weight"])
    for l in range(n_enc):
        pre, mk = f"transformer.encoder.layers.{l}.", lambda n: masks.get(("enc", l, n))  # noqa: E731
        mem = ln(mem + _drop(attn(mem, mem, pre + "self_attn.", mk("attn"), text_lengths), mk("drop1"), p), pre + "norm1")
        mem = ln(mem + _drop(ff(mem, pre, mk("ff")), mk("drop2"), p), pre + "norm2")
    mem = ln(mem, "transformer.encoder.norm")
    h = F.linear(pose.reshape(B, T, 24).to(dtype), state["pose2hidden_projection.weight"], state["pose2hidden_projection.bias"])
    for l in range(n_dec):
        pre, mk = f"transformer.decoder.layers.{l}.", lambda n: masks.get(("dec", l, n))  # noqa: E731
        h = ln(h + _drop(attn(h, h, pre + "self_attn.", mk("self_attn"), frame_lengths), mk("drop1"), p), pre + "norm1")
        h = ln(h + _drop(attn(h, mem, pre + "multihead_attn.", mk("cross_attn"), text_lengths), mk("drop2"), p), pre + "norm2")
        h = ln(h + _drop(ff(h, pre, mk("ff")), mk("drop3"), p), pre + "norm3")
    h = ln(h, "transformer.decoder.norm")
    y = F.linear(h, state["hidden2pose_projection.weight"], state["hidden2pose_projection.bias"])
    return y.reshape(B, T, 21, 2)


def grads_of(forward, tokens, pose, state, dy, dtype):
    """y, the parameter gradients (order of param_keys) and dx of sum(y * dy) through forward(tokens, x, leaves)."""
    st = leaf_state(state, dtype)
    xx = torch.as_tensor(pose).detach().to(dtype).clone().requires_grad_(True)
    y = forward(tokens, xx, st)
    (y * torch.as_tensor(dy).to(dtype)).sum().backward()
    keys = param_keys(*layer_counts(st))
    return y.detach(), [st[k].grad if st[k].grad is not None else torch.zeros_like(st[k]) for k in keys], xx.grad


def case_data(name, seed=0):
    """tokens (padded with 0 from text_lengths on), pose, dy (zero at padded frames) and the lengths of a case."""
    (B, S, T), tl, fl, _ = CASES[name]
    g = torch.Generator().manual_seed(9100 + seed + 17 * sorted(CASES).index(name))
    tok = torch.randint(1, N_TOKENS - 1, (B, S), generator=g)
    for b, n in enumerate(tl):
        tok[b, n:] = 0
    x = torch.randn((B, T, 12, 2), generator=g)
    dy = torch.randn((B, T, 21, 2), generator=g) * valid_frames(fl, T)[:, :, None, None]
    for b, n in enumerate(fl):
        x[b, n:] = 0
    return tok, x, dy, list(tl), list(fl)


def case_state(name):
    n_enc, n_dec = CASES[name][3]
    return recipe_state(9000 + 10 * n_enc + n_dec, N_TOKENS, n_enc, n_dec)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(y64, g64, dx64, err32 per gradient, err32 of dx) of a case at p = 0 from the nn.Transformer oracle in float64 and
    float32; computed once, shared, so leave it unchanged."""
    tok, x, dy, tl, fl = case_data(name)
    state = case_state(name)
    fwd = lambda dt: (lambda t, xx, st: oracle_forward(t, xx, st, tl, fl, dt))  # noqa: E731
    y64, g64, dx64 = grads_of(fwd(torch.float64), tok, x, state, dy, torch.float64)
    _, g32, dx32 = grads_of(fwd(torch.float32), tok, x, state, dy, torch.float32)
    return (y64, g64, dx64, [float((b.double() - a).abs().max()) for a, b in zip(g64, g32)],
            float((dx32.double() - dx64).abs().max()))


def port_reference(name, masks, p):
    """The same tuple from port_forward_masked with the given keep-masks (CPU), for the cases with dropout."""
    tok, x, dy, tl, fl = case_data(name)
    state = case_state(name)
    fwd = lambda dt: (lambda t, xx, st: port_forward_masked(t, xx, st, masks, p, dt, tl, fl))  # noqa: E731
    y64, g64, dx64 = grads_of(fwd(torch.float64), tok, x, state, dy, torch.float64)
    _, g32, dx32 = grads_of(fwd(torch.float32), tok, x, state, dy, torch.float32)
    return (y64, g64, dx64, [float((b.double() - a).abs().max()) for a, b in zip(g64, g32)],
            float((dx32.double() - dx64).abs().max()))


def repadded(name, seed=1):
    """The case's tokens and pose with other content in the padding: other valid ids behind text_lengths, finite random
    rows behind frame_lengths.  Nothing else differs."""
    tok, x, dy, tl, fl = case_data(name)
    g = torch.Generator().manual_seed(9500 + seed)
    tok2, x2 = tok.clone(), x.clone()
    for b, n in enumerate(tl):
        tok2[b, n:] = torch.randint(1, N_TOKENS - 1, (tok.shape[1] - n,), generator=g)
    for b, n in enumerate(fl):
        x2[b, n:] = torch.randn((x.shape[1] - n, 12, 2), generator=g) * 3
    return tok2, x2

