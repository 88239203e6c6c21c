"""The address sequence of enc_attention_x3_kernel (csrc/attention_x3.hip), without a device: wlk_diag_attn_x3_addresses
returns, from the host / device functions the kernel itself calls, every 16-byte request of one workgroup - the Q fragments
and, ring step by ring step, the LDS-DMA sources with their LDS destinations.  The kernel forms a source by advancing a
pointer and switches to a separate pointer for the last pair; this file restates the closed form it must agree with -
min((2 sc + stream) * 32 + key_row, T - 1) * row_qk for a K piece, min(sc, (n_tiles - 1 - stream) / 2) * adv for a V^T piece,
sc = min(step, n_steps - 1), slot = step % 3 - and checks the sequence against it, against the bounds of the operand image,
and for covering every slot exactly once per step.  A wrong source address on the device is a memory fault, not a wrong
number, so this runs first.

Cases: every T in 64 .. 600 with every d in {64, 128, 1280} on one workgroup each (head and query tile dealt round, the last
ones included), and every head and query tile of a few shapes.  Share of the (T, d) pairs skipped: none."""
import ctypes as C

import numpy as np
import pytest

from whisperlivekit_amd import _lib

QT, KT = 64, 32
K_ROW, V_ROW = 384, 192
K_BYTES = V_BYTES = 12288
TILE_BYTES = K_BYTES + V_BYTES
SLOT_BYTES = 2 * TILE_BYTES
NB, NPW = 3, 6
ALL_T = tuple(range(64, 601))
ALL_D = (64, 128, 1280)
EVERY_WORKGROUP = ((64, 128), (97, 64), (193, 128), (321, 1280), (449, 128), (600, 64))


def addresses(T, d, head, q_tile):
    """-> (src [n] int64, lds [n] int32, image bytes) of workgroup (head, q_tile)"""
    lib = _lib.load()
    n, image = C.c_int64(), C.c_int64()
    H = d // 64
    assert lib.wlk_diag_attn_x3_addresses(T, d, H, head, q_tile, None, None, 0, C.byref(n), C.byref(image)) == 0, lib.wlk_diag_last_error()
    src, lds = np.full(n.value, -7, np.int64), np.full(n.value, -7, np.int32)
    assert lib.wlk_diag_attn_x3_addresses(T, d, H, head, q_tile, src.ctypes.data, lds.ctypes.data, n.value, C.byref(n), None) == 0
    assert n.value == src.size
    return src, lds, image.value


def closed_form(T, d, head, q_tile):
    """the requests as the formulas of the docstring give them, in the order of wlk_diag_attn_x3_addresses"""
    n_tiles = (T + KT - 1) // KT
    n_steps = (n_tiles + 1) // 2
    vt_ld = (T + 31) // 32 * 32
    row_qk, row_vt = 3 * (2 * d) * 2, 3 * vt_ld * 2
    vt_bytes0 = 2 * (T * 3 * 2 * d)                 # the image's V^T part starts behind its T rows of q | k
    # Q fragments: thread (wave, lane), feature step, plane
    tid = np.arange(512, dtype=np.int64)
    lane, wave = tid & 63, tid >> 6
    c, g = lane & 15, lane >> 4
    q = np.minimum(q_tile * QT + 16 * (wave & 3) + c, T - 1)
    kstep, p = np.arange(2, dtype=np.int64)[None, :, None], np.arange(3, dtype=np.int64)[None, None, :]
    q_src = (q * row_qk + head * 8 * 48)[:, None, None] + ((4 * kstep + g[:, None, None]) * 3 + p) * 16
    # DMA: ring step, wave, piece, lane
    step = np.arange(n_steps + 2, dtype=np.int64)[:, None, None, None]
    wave = np.arange(8, dtype=np.int64)[None, :, None, None]
    i = np.arange(NPW, dtype=np.int64)[None, None, :, None]
    lane = np.arange(64, dtype=np.int64)[None, None, None, :]
    sc = np.minimum(step, n_steps - 1)
    byte = 1024 * (wave + 8 * i) + 16 * lane
    stream, in_tile = byte // TILE_BYTES, byte % TILE_BYTES
    is_k = in_tile < K_BYTES
    k_row = in_tile // K_ROW
    k_up = (in_tile % K_ROW) >> 4
    k_unit = ((k_up // 3) ^ (k_row & 7)) * 3 + k_up % 3
    key = np.minimum((2 * sc + stream) * KT + k_row, T - 1)
    k_src = (d // 8 + head * 8) * 48 + k_unit * 16 + key * row_qk
    off = in_tile - K_BYTES
    v_row = off // V_ROW
    v_up = (off % V_ROW) >> 4
    v_unit = ((v_up // 3) ^ ((v_row >> 1) & 3)) * 3 + v_up % 3
    adv = 2 * (KT // 8) * 48
    v_src = (vt_bytes0 + (head * 64 + v_row) * row_vt + v_unit * 16 + stream * (KT // 8) * 48 +
             np.minimum(sc, (n_tiles - 1 - stream) // 2) * adv)
    dma_src = np.where(is_k, k_src, v_src)
    dma_lds = (step % NB) * SLOT_BYTES + byte
    src = np.concatenate([q_src.reshape(-1), dma_src.reshape(-1)])
    lds = np.concatenate([np.full(q_src.size, -1, np.int64), np.broadcast_to(dma_lds, dma_src.shape).reshape(-1)])
    return src, lds, n_steps, 2 * (T * 3 * 2 * d + d * 3 * vt_ld)


def check(T, d, head, q_tile):
    src, lds, image = addresses(T, d, head, q_tile)
    want_src, want_lds, n_steps, want_image = closed_form(T, d, head, q_tile)
    who = f"T={T} d={d} head={head} q_tile={q_tile}"
    assert image == want_image, who
    assert src.size == 512 * 6 + (n_steps + 2) * 8 * NPW * 64, who
    assert np.array_equal(src, want_src), (who, int(np.argmax(src != want_src)))
    assert np.array_equal(lds, want_lds), (who, int(np.argmax(lds != want_lds)))
    # every request lies inside the image, whole and aligned
    assert src.min() >= 0 and src.max() + 16 <= image and not (src % 16).any(), who
    # every step fills each 16-byte unit - so each 1 KiB piece - of its slot exactly once, and nothing outside the ring
    dma = lds[512 * 6:].reshape(n_steps + 2, -1).astype(np.int64)
    slot = np.arange(n_steps + 2) % NB
    want = slot[:, None] * SLOT_BYTES + 16 * np.arange(SLOT_BYTES // 16)[None, :]
    assert np.array_equal(np.sort(dma, axis=1), want), who
    pieces = (dma - slot[:, None] * SLOT_BYTES) // 1024
    assert all(np.array_equal(np.bincount(row, minlength=48), np.full(48, 64)) for row in pieces), who
    assert dma.max() + 16 <= NB * SLOT_BYTES, who


@pytest.mark.parametrize("d", ALL_D)
def test_every_T_from_64_to_600(d):
    H = d // 64
    for n, T in enumerate(ALL_T):
        q_tiles = (T + QT - 1) // QT
        # dealt round, and the last head with the last (partial) query tile at every fourth T
        head, q_tile = ((H - 1, q_tiles - 1) if n % 4 == 0 else ((n * 7) % H, (n * 3) % q_tiles))
        check(T, d, head, q_tile)


@pytest.mark.parametrize("T,d", EVERY_WORKGROUP)
def test_every_workgroup_of_a_shape(T, d):
    for head in range(d // 64):
        for q_tile in range((T + QT - 1) // QT):
            check(T, d, head, q_tile)


def test_no_pair_is_skipped():
    assert ALL_T == tuple(range(64, 601)) and ALL_D == (64, 128, 1280)      # the docstring's "none"


def test_refusals():
    lib = _lib.load()
    n = C.c_int64()
    for T, d, H, head, q_tile, fragment in ((63, 64, 1, 0, 0, "unsupported shape"), (64, 128, 3, 0, 0, "unsupported shape"),
                                            (64, 128, 2, 2, 0, "no such workgroup"), (129, 64, 1, 0, 3, "no such workgroup"),
                                            (129, 64, 1, -1, 0, "no such workgroup")):
        assert lib.wlk_diag_attn_x3_addresses(T, d, H, head, q_tile, None, None, 0, C.byref(n), None) == -1
        assert fragment in lib.wlk_diag_last_error().decode(), (T, d, H, head, q_tile)
