"""The augmented batch of b2h_build_batch_aug (include/b2h.h, kernel_build_batch_aug.h) restated in numpy float32 on
tests/philox_ref.philox4x32_10, for tests/test_build_batch_aug_*.py and tests/test_graph_trainer_aug_gpu.py.  The
reference has no augmentation: this is parity with the project's own definition, never with the reference.

  draws(...)         s, c, sn, mirror of one sequence from its block (p, 16, epoch lo, epoch hi)
  virtual_rows(...)  the store rows of one sequence, mirrored, rotated and scaled about each frame's raw chest
  batch(...)         the virtual rows handed to batch_ref.batch, then the jitter on input_kp, then the division

Every operation is one numpy float32 operation (numpy fuses nothing), in the order the header states them, so a kernel
that keeps that order and contracts nothing gives the same bits.  A helper module, not a conftest.py: the tests import
it by name."""
import collections

import numpy as np
import torch

import batch_ref
import philox_ref

F = np.float32
TAG_SEQUENCE, TAG_JITTER = 16, 17
BODY_MIRROR = [0, 1, 5, 6, 7, 2, 3, 4, 9, 8, 11, 10]

# struct b2h_augment: float32 values
Params = collections.namedtuple("Params", "scale rotate_tan mirror_p jitter")


def params(augment):
    """The b2h_augment of a hand_pose_sl_amd.Augment."""
    return Params(F(augment.scale), F(augment.rotate_tan), F(augment.mirror), F(augment.jitter))


def mirror_map(n_body):
    """M: virtual joint q reads store joint M[q] under a mirror (body sides swapped, hand blocks swapped)."""
    return BODY_MIRROR[:n_body] + list(range(n_body + 21, n_body + 42)) + list(range(n_body, n_body + 21))


def unit(w):
    """d(w) = float(w >> 8) * 2^-24 * 2 - 1, in [-1, 1), exact in float32."""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(F) * F(2.0 ** -24) * F(2) - F(1)


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def draws(par, p, epoch, seed):
    """(s, c, sn, mirror) of the sequence with draw index p: float32 scalars and a bool."""
    w = philox_ref.philox4x32_10(p, TAG_SEQUENCE, epoch & 0xFFFFFFFF, (epoch >> 32) & 0xFFFFFFFF, *_key(seed))
    s = F(1) + F(par.scale) * unit(w[0])
    t = F(par.rotate_tan) * unit(w[1])
    t2 = t * t
    den = F(1) + t2
    c = (F(1) - t2) / den
    sn = (t + t) / den
    assert all(v.dtype == F for v in (s, c, sn))
    return s, c, sn, int(w[2]) < philox_ref.threshold(par.mirror_p)


def virtual_rows(rows, n_body, par, p, epoch, seed):
    """rows: (n, 3 J) float32 numpy array of ONE utterance -> its virtual rows under the draws of index p."""
    J = n_body + 42
    a = np.asarray(rows, dtype=F).reshape(-1, 3, J)
    s, c, sn, mirror = draws(par, p, epoch, seed)
    spin = float(par.scale) != 0.0 or float(par.rotate_tan) != 0.0     # a stage whose parameters are 0 is not run
    x, y, conf = a[:, 0], a[:, 1], a[:, 2]
    if mirror:
        m = mirror_map(n_body)
        x, y, conf = x[:, m], y[:, m], conf[:, m]
    if spin or mirror:
        cx, cy = a[:, 0, 1:2], a[:, 1, 1:2]                            # the raw chest, which M fixes
        dx = x - cx
        if mirror:
            dx = -dx
        if not spin:
            x = cx + dx
        else:
            dy = y - cy
            rx = c * dx - sn * dy
            ry = sn * dx + c * dy
            x = cx + s * rx
            y = cy + s * ry
    out = np.stack([x, y, conf], axis=1)
    assert out.dtype == F
    return np.ascontiguousarray(out.reshape(-1, 3 * J))


def jitter(par, p, epoch, seed, T, ni):
    """(T, ni, 2) float32: jitter * d(w) of input joint j of frame t, from the block (p, 17 | t << 8, epoch lo, j >> 1)."""
    t, j = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(ni, dtype=np.uint64), indexing="ij")
    w = philox_ref.philox4x32_10(np.full(t.shape, p, np.uint64).ravel(), (np.uint64(TAG_JITTER) | t << np.uint64(8)).ravel(),
                                 np.full(t.shape, epoch & 0xFFFFFFFF, np.uint64).ravel(), (j >> np.uint64(1)).ravel(), *_key(seed))
    odd = (j.ravel() & np.uint64(1)).astype(bool)
    wx, wy = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    return np.stack([F(par.jitter) * unit(wx), F(par.jitter) * unit(wy)], axis=-1).reshape(T, ni, 2)


def batch(rows, offsets, n_body, tokens, utt, start, T, predict="right_hand", dif=True, norm=True, factor=1280, frame0=False,
          par=Params(0, 0, 0, 0), seed=0, epoch=0, entry0=0, index=None):
    """batch_ref.batch of the same arguments under b2h_augment `par` and key (seed, epoch).  The draw index of sequence b
    is index[b], by default entry0 + b."""
    utt = [int(u) for u in utt]
    index = [entry0 + b for b in range(len(utt))] if index is None else [int(p) for p in index]
    host = rows.numpy()
    virt = [virtual_rows(host[int(offsets[u]):int(offsets[u + 1])], n_body, par, p, epoch, seed) for u, p in zip(utt, index)]
    voff = torch.tensor([0] + np.cumsum([v.shape[0] for v in virt]).tolist(), dtype=torch.int64)
    vrows = torch.from_numpy(np.concatenate(virt, axis=0))
    vtok = None if tokens is None else tokens[utt]
    out = batch_ref.batch(vrows, voff, n_body, vtok, range(len(utt)), start, T, predict, dif, False, factor, frame0)
    if float(par.jitter) != 0.0:
        kp = out["input_kp"].numpy().copy()
        for b, (u, p) in enumerate(zip(utt, index)):
            n = int(offsets[u + 1]) - int(offsets[u])
            live = T if (frame0 and n > 0) else min(n, T)              # frames of zero padding get none
            kp[b, :live] = kp[b, :live] + jitter(par, p, epoch, seed, T, kp.shape[2])[:live]
        assert kp.dtype == F
        out["input_kp"] = torch.from_numpy(kp)
    if norm:
        out["input_kp"], out["target_kp"] = out["input_kp"] / factor, out["target_kp"] / factor
    return out


def mirrors(par, seed, epoch, index):
    """The mirror outcome of every draw index of `index`."""
    return [draws(par, p, epoch, seed)[3] for p in index]
