"""Host model of the evaluation mirror's bit (include/xq_hip.h, xq_engine_init_em).  TEST INFRASTRUCTURE ONLY.

A transcription of the engine's Philox4x32-10 (`philox_u64` of csrc/xq_engine_state.cuh) and of the bit's packing, written from
the header's text in Python integers; tests/test_eval_mirror_model.py holds it against hip.eval_mirror_bit, the device's own code
run on the host."""
M32 = 0xFFFFFFFF


def philox_u64(key: int, rank: int, slot: int, kind: int, ctr: int, sub: int) -> int:
    """Key words (key low, key high), counter words (slot, kind | sub << 8, ctr, rank), ten rounds; output word 0 is the high half
    of the result and word 1 the low half."""
    c0, c1, c2, c3 = slot & M32, (kind | (sub << 8)) & M32, ctr & M32, rank & M32
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0 << 32) | c1


def mirror_bit(seed: int, rank: int, slot: int, game_seq: int, ply: int, is_root: int, sims_done: int, row: int = 0) -> int:
    h = philox_u64(seed, rank, slot, 9, game_seq, ply & 0xFFFFFF)
    r = philox_u64(h, rank, slot, 9, (int(is_root) << 31) | (row << 16) | sims_done, 0)
    return r >> 63


def mirror_action(a: int) -> int:
    """Both squares' columns c -> 8 - c."""
    frm, to = divmod(a, 90)
    return ((frm // 9) * 9 + 8 - frm % 9) * 90 + (to // 9) * 9 + 8 - to % 9
