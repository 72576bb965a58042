"""CPU: the numpy Philox4x32-10 of tests/philox_ref.py (the GPU mask tests lean on it) is the standard generator, and its masks have the shape,
the keep rate and the counter fold the GPU tests assume."""
import torch

from tests.philox_ref import philox4x32_10, host_ln_mask, host_attn_mask


def test_host_philox_known_answers():
    """Random123's published vectors for philox4x32_10 (kat_vectors)"""
    def one(ctr, key):
        return [int(v) for v in philox4x32_10(*ctr, key[0] | (key[1] << 32))]
    assert one((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert one((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert one((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_host_masks_shape_rate_and_counter():
    m = host_ln_mask(64, 256, 0.1, 1234)
    assert m.shape == (64, 256) and m.dtype == torch.float32 and abs(m.mean().item() - 0.9) <= 5 * (0.09 / m.numel()) ** 0.5
    a = host_attn_mask(2, 37, 3, 0.1, 11)
    assert a.shape == (2, 3, 37, 37) and a.dtype == torch.uint8 and abs(a.float().mean().item() - 0.9) <= 5 * (0.09 / a.numel()) ** 0.5
    assert torch.equal(a, host_attn_mask(2, 37, 3, 0.1, 11, 0)) and not torch.equal(a, host_attn_mask(2, 37, 3, 0.1, 11, 1))
    assert torch.equal(m, host_ln_mask(64, 256, 0.1, 1234, 0)) and not torch.equal(m, host_ln_mask(64, 256, 0.1, 1235))
    assert host_attn_mask(1, 4, 1, 0.0, 5).all()                     # p = 0: threshold 0, nothing dropped
