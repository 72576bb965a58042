"""Host restatement of csrc/dropout.h: the keep masks that the kernels regenerate from Philox4x32-10 (test infrastructure, the role of
tests/bert_ref.py).  include/act_hip.h documents the keys -- (seed, row, column / 4) and (seed, (b H + h) S + query, key / 4); the counter layout,
the domain words, the fold of the device-resident counter into the seed and the 24-bit drop threshold are read off dropout.h and pinned here on
purpose: a key shift shared by a forward and its backward changes no seeded-versus-injected comparison, only this one.
tests/test_philox_host.py pins the generator itself to Random123's known answers."""
import numpy as np
import torch

# counter word c2, the table of csrc/dropout.h: a new user takes the next free value and adds its line in both files
PHILOX_DOMAIN_GUMBEL, PHILOX_DOMAIN_ROWS, PHILOX_DOMAIN_ATTN, PHILOX_DOMAIN_AUGMENT = 0, 1, 2, 3


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 numpy arrays holding 32-bit words; key = (seed low, seed high) -> four words per counter"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack((c0, c1, c2, c3), axis=-1)


def _fold_counter(seed, ctr):
    return seed if ctr is None else seed ^ ((ctr * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _threshold(p):
    return np.uint64(int(np.float32(p) * np.float32(16777216.0)))          # an entry is dropped when its top 24 random bits are below this


def host_ln_mask(T, D, p, seed, ctr=None):
    """the domain-1 stream of EVERY dense-row user (dropout.h: dropout_dropped4 -- prompt_rows, prompt_layernorm, prompt_kv, dropout_add_layernorm):
    keyed by (seed, row, column / 4) as include/act_hip.h says; counter words (column / 4, row, PHILOX_DOMAIN_ROWS, 0), one output word per
    channel of the float4"""
    r = philox4x32_10(np.arange(D // 4)[None, :], np.arange(T)[:, None], PHILOX_DOMAIN_ROWS, 0, _fold_counter(seed, ctr))        # [T, D/4, 4]
    return torch.from_numpy(((r >> np.uint64(8)) >= _threshold(p)).reshape(T, D).astype(np.float32))


def host_attn_mask(B, S, H, p, seed, ctr=None):
    """dropout.h, dropout_attn_keep4 / dropout_attn_keep1: keyed by (seed, (b H + h) S + query, key / 4) as include/act_hip.h says; counter words
    (key / 4, row id, PHILOX_DOMAIN_ATTN, 0)"""
    nk = (S + 3) // 4
    r = philox4x32_10(np.arange(nk)[None, :], np.arange(B * H * S)[:, None], PHILOX_DOMAIN_ATTN, 0, _fold_counter(seed, ctr))   # [B H S, nk, 4]
    keep = ((r >> np.uint64(8)) >= _threshold(p)).reshape(B * H * S, nk * 4)[:, :S]
    return torch.from_numpy(np.ascontiguousarray(keep).astype(np.uint8)).view(B, H, S, S)
