"""A numpy restatement, on the host, of whole-store inference over overlapping windows -- written for the tests of
b2h_window_plan_overlap and b2h_scatter_rows_blend from their contracts in include/b2h.h:

  plan(...)       windows of T frames at stride T - K, the last a full window that ends with the utterance
  owned(...)      which (entry, frame) writes which row, and for the frames of a blend region the predecessor's frame,
                  the position p and the width w
  scatter(...)    the predictions of a whole plan written back: per value the blend (LINEAR: three float32 operations
                  after the float32 division of the weights; CENTRE: a select), then tests/rows_ref.py's
                  fl(fl(v * factor) + wrist), and which words were addressed

Every arithmetic step is one numpy float32 operation in the order the header states, so the kernel is held to it bit for
bit; the result cannot depend on how a caller cuts the plan into batches, since there is no batch here.  A helper module,
not a conftest.py: the tests import it by name.
"""
import numpy as np

from batch_ref import TARGET
from rows_ref import DIF, NORMALIZE

LINEAR, CENTRE = 0, 1          # enum b2h_blend


def plan(lengths, T, K):
    """(utt, start, skip) as lists, for utterances of `lengths` rows."""
    s = T - K
    utt, start, skip = [], [], []
    for u, L in enumerate(int(v) for v in lengths):
        if L == 0:
            continue
        if L <= T:
            entries = [(0, 0)]
        else:
            n = -(-(L - T) // s) + 1
            entries = [(i * s, 0) for i in range(n - 1)] + [(L - T, (n - 1) * s - (L - T))]
        for a, k in entries:
            utt.append(u), start.append(a), skip.append(k)
    return utt, start, skip


def _window(offsets, u, start, T, n_rows):
    """(first row of the utterance, its length, the clamped start), or None for an id that addresses nothing."""
    if not 0 <= u < len(offsets) - 1:
        return None
    r0, r1 = int(offsets[u]), int(offsets[u + 1])
    if r0 < 0 or r1 < r0 or (n_rows is not None and r1 > n_rows):
        return None
    L = r1 - r0
    return r0, L, (min(max(int(start), 0), L - T) if L > T else 0)


def owned(offsets, utt, start, skip, T, n_rows=None):
    """[(e, t, row, blend)] of every frame the write-back of the plan writes, in (e, t) order; blend is None outside a
    blend region, else (predecessor's frame, p, w)."""
    out = []
    for e, u in enumerate(int(v) for v in utt):
        win = _window(offsets, u, start[e], T, n_rows)
        if win is None:
            continue
        r0, L, s = win
        k = max(int(skip[e]), 0)
        end = min(L, T)
        if e + 1 < len(utt) and int(utt[e + 1]) == u:
            s2 = _window(offsets, u, start[e + 1], T, n_rows)[2]
            end = min(end, s2 + max(int(skip[e + 1]), 0) - s)
        w, s0 = 0, None
        if e > 0 and int(utt[e - 1]) == u:
            s0 = _window(offsets, u, start[e - 1], T, n_rows)[2]
            w = max(s0 + T - (s + k), 0)
        for t in range(k, end):
            p = t - k
            blend = (t + s - s0, p, w) if p < w and t + s - s0 >= 0 else None
            out.append((e, t, r0 + s + t, blend))
    return out


HALO_SEED = 3                  # of the ConvModel whose window seams the halo tests measure (torch.manual_seed)
HALO_OFFSETS = [0, 70, 140, 210]


def halo_rows():
    """The store of the halo tests: three utterances of 70 rows, 12 body joints, every value uniform in [0, 1) -- the
    unit scale at which the project's fp32 parity bar of 2e-5 is stated, so that with normalize=False the model runs
    in the units the bar is for."""
    return np.random.default_rng(70).random((210, 162), dtype=np.float32)


def windowed(forward, rows, T, K, blend):
    """The halo store predicted by `forward` ((B, T, 12, 2) float32 numpy -> (B, T, 21, 2)) over the windows of
    plan(T, K), all in one batch, and written back without transforms (flags 0): (210, 162) float32."""
    utt, start, skip = plan(np.diff(HALO_OFFSETS), T, K)
    x = np.stack([np.stack([rows[HALO_OFFSETS[u] + s:HALO_OFFSETS[u] + s + T, :12],
                            rows[HALO_OFFSETS[u] + s:HALO_OFFSETS[u] + s + T, 54:66]], axis=2) for u, s in zip(utt, start)])
    preds = np.ascontiguousarray(forward(x), dtype=np.float32)
    return scatter(rows, HALO_OFFSETS, 12, utt, start, skip, T, "right_hand", 0, 1.0, preds, blend, 1.0, rows)[0]


def near_seams(T, L=70, halo=8):
    """Bool (210,): the rows within `halo` frames of a boundary between the touching windows of plan(T, 0)."""
    near = np.zeros(HALO_OFFSETS[-1], bool)
    utt, start, skip = plan(np.diff(HALO_OFFSETS), T, 0)
    for u, s, k in zip(utt, start, skip):
        if s + k > 0:
            seam = HALO_OFFSETS[u] + s + k
            near[max(seam - halo, HALO_OFFSETS[u]):min(seam + halo, HALO_OFFSETS[u + 1])] = True
    return near


def scatter(rows, offsets, n_body, utt, start, skip, T, predict, flags, factor, preds, blend, conf, rows_out):
    """(rows_out after the write-back of the whole plan, bool array of the words it addressed, bool array of the rows
    that lie in a blend region).  preds: (n_plan, T, nt, 2) float32 numpy, the prediction of every entry."""
    J = n_body + 42
    d = np.arange(TARGET[predict].start, TARGET[predict].stop) + n_body + 21
    out, hit, mixed = rows_out.copy(), np.zeros(rows_out.shape, bool), np.zeros(rows_out.shape[0], bool)
    f, one = np.float32(factor), np.float32(1)
    for e, t, row, region in owned(offsets, utt, start, skip, T, rows.shape[0]):
        v = preds[e, t].astype(np.float32)                              # (nt, 2)
        if region is not None:
            ta, p, w = region
            pa = preds[e - 1, ta].astype(np.float32)
            if blend == LINEAR:
                wb = np.float32(p + 1) / np.float32(w + 1)
                wa = one - wb
                v = wa * pa + wb * v
            elif 2 * p < w:
                v = pa
            mixed[row] = True
        x, y = v[:, 0], v[:, 1]
        if flags & NORMALIZE:
            x, y = x * f, y * f
        if flags & DIF:
            x, y = x + rows[row, 4], y + rows[row, J + 4]
        assert x.dtype == np.float32 and y.dtype == np.float32
        assert not hit[row, d].any(), "a row with two writers"
        out[row, d], out[row, J + d], out[row, 2 * J + d] = x, y, np.float32(conf)
        hit[row, d] = hit[row, J + d] = hit[row, 2 * J + d] = True
    return out, hit, mixed
