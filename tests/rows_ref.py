"""A numpy restatement, on the host, of whole-store inference -- written for the tests of b2h_window_plan,
b2h_scatter_rows and b2h_joint_error from their contracts in include/b2h.h:

  plan(...)         the windows that cover every frame of every utterance once (or the first window of each)
  scatter(...)      a batch of predictions written back into store rows: the window of tests/batch_ref.py's `item`, then
                    per value fl(fl(p * factor) + wrist) as separate float32 operations, and which words were addressed
  joint_error(...)  per utterance and right-hand joint, the float32 sum in ascending row order of
                    sqrt(fl(fl(dx dx) + fl(dy dy))) over the rows whose true confidence is > 0, and their count

Every arithmetic step is one numpy float32 operation in the order the header states, so the kernels are held to it bit for
bit.  A helper module, not a conftest.py: the tests import it by name.
"""
import numpy as np

from batch_ref import TARGET

NORMALIZE, DIF = 2, 1          # B2H_BATCH_NORMALIZE, B2H_BATCH_DIF_ENCODING


def plan(lengths, T, coverage="all"):
    """(utt, start, skip) as lists, for utterances of `lengths` rows."""
    utt, start, skip = [], [], []
    for u, L in enumerate(int(v) for v in lengths):
        if L == 0:
            continue
        if coverage == "first" or L <= T:
            entries = [(0, 0)]
        else:
            k = -(-L // T)
            entries = [(i * T, 0) for i in range(k - 1)] + [(L - T, k * T - L)]
        for s, k in entries:
            utt.append(u), start.append(s), skip.append(k)
    return utt, start, skip


def addressed_rows(offsets, utt, start, skip, T, n_rows=None):
    """[(b, t, row)] of every frame a write-back of this batch writes, in (b, t) order; an id outside the store, or
    offsets of it outside 0 <= lo <= hi <= n_rows, addresses nothing."""
    n_utt, out = len(offsets) - 1, []
    for b, u in enumerate(int(v) for v in utt):
        if not 0 <= u < n_utt:
            continue
        r0, r1 = int(offsets[u]), int(offsets[u + 1])
        if r0 < 0 or r1 < r0 or (n_rows is not None and r1 > n_rows):
            continue
        L = r1 - r0
        s = min(max(0 if start is None else int(start[b]), 0), L - T) if L > T else 0
        first = 0 if skip is None else max(int(skip[b]), 0)
        out += [(b, t, r0 + s + t) for t in range(first, min(L, T))]
    return out


def scatter(rows, offsets, n_body, utt, start, skip, T, predict, flags, factor, pred, conf, rows_out):
    """(rows_out after the write-back, bool array of the words it addressed).  rows, rows_out: (N, 3 J) float32 numpy;
    pred (B, T, nt, 2) float32 numpy; start, skip: sequences or None."""
    J = n_body + 42
    d = np.arange(TARGET[predict].start, TARGET[predict].stop) + n_body + 21
    out, hit = rows_out.copy(), np.zeros(rows_out.shape, bool)
    f = np.float32(factor)
    for b, t, row in addressed_rows(offsets, utt, start, skip, T, rows.shape[0]):
        x, y = pred[b, t, :, 0].astype(np.float32), pred[b, t, :, 1].astype(np.float32)
        if flags & NORMALIZE:
            x, y = x * f, y * f
        if flags & DIF:
            x, y = x + rows[row, 4], y + rows[row, J + 4]
        assert x.dtype == np.float32 and y.dtype == np.float32
        out[row, d], out[row, J + d], out[row, 2 * J + d] = x, y, np.float32(conf)
        hit[row, d] = hit[row, J + d] = hit[row, 2 * J + d] = True
    return out, hit


def joint_error(rows_pred, rows_true, offsets, n_body):
    """(utt_sum (U, 21) float32, utt_count (U, 21) int32)."""
    J, h = n_body + 42, n_body + 21
    n_utt = len(offsets) - 1
    utt_sum, utt_count = np.zeros((n_utt, 21), np.float32), np.zeros((n_utt, 21), np.int32)
    for u in range(n_utt):
        for row in range(int(offsets[u]), int(offsets[u + 1])):
            p, q = rows_pred[row], rows_true[row]
            dx, dy = p[h:h + 21] - q[h:h + 21], p[J + h:J + h + 21] - q[J + h:J + h + 21]
            dist = np.sqrt(dx * dx + dy * dy)
            assert dist.dtype == np.float32
            counted = q[2 * J + h:2 * J + h + 21] > 0
            utt_sum[u] = np.where(counted, utt_sum[u] + dist, utt_sum[u])
            utt_count[u] += counted
    return utt_sum, utt_count


def same_bits(a, b):
    """Equal shape, dtype and bit patterns of two numpy arrays."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
