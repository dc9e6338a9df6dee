"""Inputs shared by the decode-attention tests (CPU and GPU).

D = 128, Hkv = 2. Every position >= seq_lens[b] of k and v is NaN: an
output that is not finite means a masked slot leaked. All values are exact
in bf16.
"""

import numpy as np

D = 128
HKV = 2


def v_code(batch, lmax):
    """v[b, h, pos, d] = ((7*pos + 3*d + 5*h + 11*b) % 251) - 125: integers
    with |v| <= 125, so any wrong batch, head, position or d index shows."""
    b, h, pos, d = np.ogrid[:batch, :HKV, :lmax, :D]
    return (((7 * pos + 3 * d + 5 * h + 11 * b) % 251) - 125).astype(
        np.float32)


def nan_tail(x, seq_lens):
    for b, n in enumerate(seq_lens):
        x[b, :, n:] = np.nan
    return x


def onehot_keys(batch, lmax):
    """k[..., pos, pos % 64] = k[..., pos, 64 + pos // 64] = 1, else 0."""
    k = np.zeros((batch, HKV, lmax, D), np.float32)
    pos = np.arange(lmax)
    k[:, :, pos, pos % 64] = 1
    k[:, :, pos, 64 + pos // 64] = 1
    return k


def onehot_targets(group, seq_lens):
    """t[b, h] = (5*h + 3*b + len - 1) % len for each of the Hq heads."""
    h = np.arange(group * HKV)
    return np.stack([(5 * h + 3 * b + n - 1) % n
                     for b, n in enumerate(seq_lens)])


def onehot_case(group, seq_lens, lmax):
    """(q, k, v, targets): head h of sequence b has q = 512 at the two hot
    coordinates of position t[b, h], so that score leads every other by
    512/sqrt(128) = 45.25 and every other weight is at most e^-45."""
    batch = len(seq_lens)
    t = onehot_targets(group, seq_lens)
    q = np.zeros((batch, group * HKV, D), np.float32)
    bi, hi = np.indices(t.shape)
    q[bi, hi, t % 64] = 512
    q[bi, hi, 64 + t // 64] = 512
    k = nan_tail(onehot_keys(batch, lmax), seq_lens)
    v = nan_tail(v_code(batch, lmax), seq_lens)
    return q, k, v, t


def uniform_case(group, seq_lens, lmax):
    """(q, k, v) with q = 0: every probability is 1/len, o is the mean of
    the first len rows of v and lse = log(len)."""
    batch = len(seq_lens)
    q = np.zeros((batch, group * HKV, D), np.float32)
    k = nan_tail(onehot_keys(batch, lmax), seq_lens)
    v = nan_tail(v_code(batch, lmax), seq_lens)
    return q, k, v
