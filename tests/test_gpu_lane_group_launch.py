"""The lane-form leaf hash as ONE grid over the commitments of a group (leaf_hash_lane_kernel with grid.y = commitment, the launch a
proof pool makes for a lane-form group), through the kernel-level entry Prover.leaf_hash_lane_group: 1 .. 4 segments of different data,
one wave, two waves, a whole workgroup and two workgroups of leaves per segment, a short, an exact and a one-over last absorb.  Every
digest equals the per-commitment lane launch of the same matrix AND the host sponge (starkhip_poseidon_permute_host, poseidon_host.cpp)
on the same rows; a changed cell changes the digest of its own leaf in its own segment and nothing else.

A leaf count is a power of two by construction (the tree order of the digests is a bit reversal over log2(leaves) bits), so the count of
192 leaves the grouped launch was first specified with cannot be launched: the entry refuses it, and the test says so.  Workgroups hold
four waves and every segment has workgroups of its own (grid.y), so no workgroup spans two segments; 256 and 512 leaves take its place."""
import numpy as np
import pytest

import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu
P = S.P
SEGMENTS = 4
MAX_LEAVES = 512
COLUMN_COUNTS = [7, 8, 9, 16, 17]   # a short absorb, an exact one, one more; two exact ones, and one more
RATE_BITS = 2


@pytest.fixture(scope="module")
def cells():
    """[segment][column][leaf]: different random cells in every segment, with 0 and p - 1 in every segment, in the first and last leaf,
    in the first column, the last column of a full absorb and the columns after it"""
    rng = np.random.default_rng(0x1A9E)
    m = rng.integers(0, P, size=(SEGMENTS, max(COLUMN_COUNTS), MAX_LEAVES), dtype=np.uint64)
    for s in range(SEGMENTS):
        for k, c in enumerate((0, 6, 7, 8, 15, 16)):
            m[s, c, (s + 3 * k) % 64] = 0 if (s + k) % 2 else P - 1
            m[s, c, 63 - (s + k) % 7] = P - 1 if (s + k) % 2 else 0
    m[0, :, 0] = P - 1   # a whole leaf of p - 1, a whole leaf of zeros
    m[1, :, 1] = 0
    return m


_sponges = {}


def host_digest(cells, seg, n_cols, leaf):
    """the sponge of hash_n_to_hash_no_pad (overwrite mode, rate 8) over cells[seg, :n_cols, leaf], on the host"""
    key = (seg, n_cols, leaf)
    if key not in _sponges:
        row = cells[seg, :n_cols, leaf]
        state = np.zeros(12, dtype=np.uint64)
        for at in range(0, n_cols, 8):
            block = row[at:at + 8]
            state[:block.size] = block
            state = S.api.poseidon_permute_host(state)
        _sponges[key] = state[:4].copy()
    return _sponges[key]


def tree_index(q, log_n, rate_bits):
    """where the digest of leaf q of a coset-major matrix goes (kernels_hash.hip)"""
    i = ((q & ((1 << log_n) - 1)) << rate_bits) + (q >> log_n)
    return int(format(i, "0%db" % (log_n + rate_bits))[::-1], 2)


def expected(cells, segs, n_cols, leaves, rate_bits):
    log_n = leaves.bit_length() - 1 - rate_bits
    want = np.zeros((segs, leaves, 4), dtype=np.uint64)
    for s in range(segs):
        for q in range(leaves):
            want[s, tree_index(q, log_n, rate_bits)] = host_digest(cells, s, n_cols, q)
    return want


@pytest.mark.parametrize("leaves", [64, 128, 256, 512])
@pytest.mark.parametrize("segs", [1, 2, 3, 4])
def test_grouped_launch_equals_single_launches_and_the_host_sponge(prover, cells, segs, leaves):
    for n_cols in COLUMN_COUNTS:
        mats = np.ascontiguousarray(cells[:segs, :n_cols, :leaves])
        log_n = leaves.bit_length() - 1 - RATE_BITS
        grouped = prover.leaf_hash_lane_group(mats, log_n, RATE_BITS, grouped=True)
        single = prover.leaf_hash_lane_group(mats, log_n, RATE_BITS, grouped=False)
        what = "%d segments x %d leaves x %d columns" % (segs, leaves, n_cols)
        assert np.array_equal(grouped, single), what + ": the grouped launch differs from the per-commitment launches"
        assert np.array_equal(grouped, expected(cells, segs, n_cols, leaves, RATE_BITS)), what + ": differs from the host sponge"
        assert (grouped < P).all()


def test_rate_bits_zero_and_a_leaf_count_that_is_no_power_of_two(prover, cells):
    mats = np.ascontiguousarray(cells[:3, :9, :128])
    got = prover.leaf_hash_lane_group(mats, 7, 0, grouped=True)
    assert np.array_equal(got, expected(cells, 3, 9, 128, 0))
    with pytest.raises(S.StarkhipError) as e:   # 192 leaves: no bit reversal, no launch
        prover.leaf_hash_lane_group(np.ascontiguousarray(cells[:2, :9, :192]), 7, 0, grouped=True)
    assert e.value.code == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:   # five segments: more than a group holds
        prover.leaf_hash_lane_group(np.ascontiguousarray(np.concatenate([cells[:, :9, :64], cells[:1, :9, :64]])), 4, 2, grouped=True)
    assert e.value.code == S.ERR_BAD_SHAPE


@pytest.mark.parametrize("seg,col,leaf", [(0, 0, 0), (2, 8, 70), (3, 16, 127), (1, 7, 64)])
def test_a_changed_cell_changes_its_own_leaf_in_its_own_segment_only(prover, cells, seg, col, leaf):
    mats = np.ascontiguousarray(cells[:, :17, :128])
    log_n = 7 - RATE_BITS
    before = prover.leaf_hash_lane_group(mats, log_n, RATE_BITS, grouped=True)
    mats[seg, col, leaf] = (int(mats[seg, col, leaf]) + 1) % P
    after = prover.leaf_hash_lane_group(mats, log_n, RATE_BITS, grouped=True)
    changed = np.argwhere((before != after).any(axis=2))
    assert changed.tolist() == [[seg, tree_index(leaf, log_n, RATE_BITS)]]
