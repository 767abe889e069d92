"""The numpy side of the gradient-loop tests (test_sac_train_host.py, test_sac_train_device.py): csrc/mjs_sac_train.h restated - the counter
layout and Philox4x32-10 in integers, the draws and ring rows they give, and the Box-Muller lines in float64 and in float32."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """``counter``: uint32 [..., 4], ``key``: (k0, k1) -> uint32 [..., 4]. Integers only (uint64 products, masked)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for r in range(10):
        if r > 0:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def row_words(B, block, step, seed):
    """The four words of every batch row's Philox block: counter (b, block, step lo, step hi), key (seed lo, seed hi)."""
    step, seed = int(step), int(seed)
    counter = np.zeros((B, 4), np.uint32)
    counter[:, 0] = np.arange(B, dtype=np.uint32)
    counter[:, 1] = block
    counter[:, 2] = step & 0xFFFFFFFF
    counter[:, 3] = step >> 32
    return philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))


def draws(B, step, seed):
    """int64 [B] below 2^62 from block 0's words w0, w1."""
    w = row_words(B, 0, step, seed).astype(np.uint64)
    return (((w[:, 0] << np.uint64(32)) | w[:, 1]) >> np.uint64(2)).astype(np.int64)


def indices(draw, size):
    return draw % size if size > 0 else np.full(draw.shape, -1, np.int64)


def normal_words(B, A, step, seed, which):
    """(first words, second words) uint32 [B, A] of every component's Box-Muller pair; ``which``: "z_next" (blocks 1, 2) or "z_pi" (3, 4).
    Component j of block k uses the pair (w0, w1) for j % 4 < 2 and (w2, w3) otherwise; even components take the cosine."""
    first = {"z_next": 1, "z_pi": 3}[which]
    w = np.concatenate([row_words(B, first, step, seed), row_words(B, first + 1, step, seed)], axis=1)  # [B, 8]
    a = np.stack([w[:, (j // 2) * 2] for j in range(A)], axis=1)
    b = np.stack([w[:, (j // 2) * 2 + 1] for j in range(A)], axis=1)
    return a, b


def box_muller(a, b, dtype):
    """The header's lines on word pairs (a, b) [B, A] in ``dtype`` (float64: exact uniforms and the true 2 pi; float32: one rounding per line,
    2 pi rounded to float32). Even columns take r cos, odd columns r sin."""
    f = dtype
    u1 = ((a >> np.uint32(8)).astype(np.uint32) + np.uint32(1)).astype(f) * f(2.0 ** -24)
    u2 = (b >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    l = np.log(u1)
    m = f(-2.0) * l
    r = np.sqrt(m)
    ang = f(6.283185307179586) * u2
    assert l.dtype == r.dtype == ang.dtype == f
    even = (np.arange(a.shape[1]) % 2 == 0)[None, :]
    return np.where(even, r * np.cos(ang), r * np.sin(ang)).astype(f)


def normals(B, A, step, seed, which, dtype=np.float32):
    return box_muller(*normal_words(B, A, step, seed, which), dtype)
