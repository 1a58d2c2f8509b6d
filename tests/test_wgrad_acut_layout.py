"""CPU model of the A piece buffer of wgrad_tiled3_acut_kernel (csrc/gs_split.hip): who writes which byte, who reads it, and which
LDS banks a wave instruction touches.  The constants are read from the kernel's source, the index maps are restated here.

LDS model (CDNA4): 64 banks of 4 bytes.  A ds_read_b128 of a wave is served in four groups of 16 lanes -- {0-3, 12-15, 20-27},
{4-11, 16-19, 28-31} and the same + 32 -- a ds_write_b64 in four groups of 16 consecutive lanes; only lanes of one group can
conflict.  Stores are also checked with the bank index folded to 32 ((addr / 4) mod 32): 16 lanes that write the SAME 8-byte
half of 16-byte units can reach at most 8 distinct 8-byte bank pairs of 16 there, whatever the layout (the pair index is
2 * unit + half with the half fixed), so two lanes per bank is the floor of that model for a wave-uniform k chunk, and what the
test pins."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "graphsage_amd", "csrc", "gs_split.hip")).read()


def _define(name):
    return int(re.search(r"^#define %s (\d+)\b" % name, SRC, re.M).group(1))


LDA, NA, NB, NR, KS = (_define(n) for n in ("W3A_LDA", "W3A_NA", "W3A_NB", "W3A_NR", "W3_KS"))
PLANE = 64 * LDA * 2                 # bytes of one piece plane: 64 m rows
A_BYTES = 3 * PLANE
B_BYTES = KS * 128 * 4
READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = READ_GROUPS + [[l + 32 for l in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]


def write_addr(wave, lane, piece):
    """Thread (wave, lane) owns column m = lane and k rows 4 wave .. 4 wave + 3: one 8-byte store per piece."""
    return piece * PLANE + (lane * LDA + 4 * wave) * 2


def read_addr(lane, i, piece):
    """Lane (l31 = lane & 31, lh = lane >> 5) of any wave: row block i, the 8 k from 8 lh of row m = 32 i + l31: 16 bytes."""
    return piece * PLANE + ((32 * i + (lane & 31)) * LDA + 8 * (lane >> 5)) * 2


def test_constants_are_the_kernels():
    assert (KS, NA, NB, NR) == (16, 2, 4, 4)
    assert re.search(r"#define W3A_LDS_BYTES \(W3A_NA \* 3 \* 64 \* W3A_LDA \* 2 \+ W3A_NB \* W3_KS \* 128 \* 4\)", SRC)
    assert (LDA * 2) % 16 == 0, "fragment reads are 16-byte aligned"


def test_every_piece_element_is_written_once_and_read_by_the_lane_that_needs_it():
    owner = {}                                        # byte -> (piece, m, k, byte of the bf16)
    for wave in range(4):
        for lane in range(64):
            for p in range(3):
                a = write_addr(wave, lane, p)
                assert a % 8 == 0 and a + 8 <= A_BYTES
                for b in range(8):                    # u32 j of the store = the pair (k0 + 2 j, k0 + 2 j + 1), low half first
                    assert a + b not in owner, "two stores overlap"
                    owner[a + b] = (p, lane, 4 * wave + b // 2, b % 2)
    elems = {v[:3] for v in owner.values()}
    assert len(owner) == 3 * 64 * KS * 2 and elems == {(p, m, k) for p in range(3) for m in range(64) for k in range(KS)}
    for lane in range(64):
        for i in range(2):
            for p in range(3):
                a = read_addr(lane, i, p)
                assert a % 16 == 0
                got = [owner[a + b] for b in range(16)]
                m, k0 = 32 * i + (lane & 31), 8 * (lane >> 5)
                assert got == [(p, m, k0 + b // 2, b % 2) for b in range(16)]      # MFMA operand order: 8 consecutive k


def _banks(addr, nbytes, nbanks):
    return [(addr // 4 + j) % nbanks for j in range(nbytes // 4)]


def test_fragment_reads_are_conflict_free():
    for i in range(2):
        for p in range(3):
            for grp in READ_GROUPS:
                hit = [b for lane in grp for b in _banks(read_addr(lane, i, p), 16, 64)]
                assert sorted(hit) == list(range(64)), "row block %d piece %d lanes %r" % (i, p, grp)


def test_piece_writes_touch_each_bank_at_most_once():
    for wave in range(4):
        for p in range(3):
            for grp in WRITE_GROUPS:
                hit = [b for lane in grp for b in _banks(write_addr(wave, lane, p), 8, 64)]
                assert len(set(hit)) == len(hit) == 32, "wave %d piece %d lanes %r" % (wave, p, grp)
                folded = np.bincount([b % 32 for b in hit], minlength=32)
                assert folded.max() <= 2, (wave, p, grp, folded)


def test_lds_budget():
    total = NA * A_BYTES + NB * B_BYTES
    assert total == 51200 and total <= 53248, "a host workgroup leaves room for two rider workgroups on its CU"
    assert 4 * 64 * 36 * 4 <= total, "the epilogue's four wave-private staging tiles overlay the buffers"
