"""The accessors that say what a launch produced (include/dxv.h: dxv_grid_count, dxv_grid_download_packed, dxv_scene_checksum; the kernels
of csrc/grid_utils.hip) against numpy and nothing else, on grids and buffers WRITTEN by the test: a voxel is solid iff its byte is
non-zero (csrc/dxv_solid.h), whatever the byte and wherever in the grid it lies -- in the 16-byte body, in the ragged tail, in the second
and third pass of the kernels' stride loops -- with three frames sharing the context's count and bit buffers, and with every other
consumer of the grid agreeing on the number."""
import ctypes as C

import numpy as np
import pytest

from raycast_restated import write_grid

pytestmark = pytest.mark.gpu

# (N, z0, nz): 4 voxels (tail only) | 8 | 108 = 6 * 16 + 12 | 700 | one pass | 258^3 = 17,173,512 bytes: the smallest even grid that takes
# k_pack_bits' stride loop (4096 workgroups x 256 lanes x 16 bytes = 256^3) into a second pass, k_count's (2048 workgroups) into a
# third, and has a ragged tail (8 bytes) behind them
SIZES = [(2, 0, 1), (2, 0, 2), (6, 1, 3), (10, 0, 7), (64, 0, 64), (258, 0, 258)]
KINDS = ["random", "all 0xFF", "all 0x02", "all 0x80", "last voxel 0x02", "voxel 0 0xFF", "planted"]
ODD = np.array([1, 2, 3, 0x80, 0xFE, 0xFF], np.uint8)
PASS = 16 * 4096 * 256                                                 # bytes of one pass of k_pack_bits' loop
PLANT = np.array([0x02, 0x00, 0x80, 0xFF, 0x00, 0x00, 0xFE, 0x04, 0x03, 0x00, 0x40, 0x00, 0x01, 0x10, 0x00, 0x7F] * 2, np.uint8)


@pytest.fixture(scope="module")
def dxv(dxvlib):
    import dxrvoxelizer_amd
    return dxrvoxelizer_amd


@pytest.fixture(scope="module")
def v(dxv, bunny):
    vb, ib, _ = bunny
    vox = dxv.Voxelizer(0)
    vox.InitFromArrays(vb, ib)
    yield vox
    vox.close()


def random_bytes(n, seed):
    """half the voxels zero; of the others half from {1, 2, 3, 0x80, 0xFE, 0xFF} and half uniform in 1 .. 255"""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, 256, n, dtype=np.uint8)
    pick = rng.random(n)
    odd = pick < 0.25
    g[odd] = ODD[rng.integers(0, len(ODD), int(odd.sum()))]
    g[pick >= 0.5] = 0
    return g


def plant(g):
    """a known pattern in the last 24 bytes (the last whole 16-byte piece and the tail behind it) and in the first two pieces of the
    second pass"""
    g[-24:] = PLANT[:24]
    g[PASS:PASS + 32] = PLANT[::-1]
    return g


def written_grid(kind, n):
    if kind == "random":
        g = random_bytes(n, 7 + n)
        return plant(g) if n >= PASS + 32 else g
    if kind.startswith("all "):
        return np.full(n, int(kind[4:], 16), np.uint8)
    g = np.zeros(n, np.uint8)
    if kind == "last voxel 0x02":
        g[-1] = 0x02
    elif kind == "voxel 0 0xFF":
        g[0] = 0xFF
    else:
        plant(g)
    return g


def check_accessors(v, g, what):
    count, bits = v.CountSolid(), v.GridBits()
    want = np.packbits(g.reshape(-1) != 0, bitorder="little")
    print(f"{what}: count {count} (numpy {int(np.count_nonzero(g))}), bit bytes that differ {int((bits != want).sum()) if bits.shape == want.shape else 'shape'}")
    assert count == int(np.count_nonzero(g)), what
    assert bits.dtype == np.uint8 and bits.shape == want.shape, what
    assert np.array_equal(bits, want), what


# ---- count and bits equal numpy on written grids -------------------------------------------------------------------------------------
# ("planted": the pattern alone in a grid of zeros, where the grid reaches the second pass; "random" carries it there as well)
CASES = [(N, z0, nz, kind) for N, z0, nz in SIZES for kind in KINDS if kind != "planted" or N * N * nz >= PASS + 32]


@pytest.mark.parametrize("N,z0,nz,kind", CASES)
def test_count_and_bits_of_written_grids_equal_numpy(v, N, z0, nz, kind):
    n = N * N * nz
    v.Voxelize(N, 0, z0, nz, frameIndex=0)
    g = written_grid(kind, n).reshape(nz, N, N)
    write_grid(v, g)
    assert np.array_equal(v.Grid(), g)
    check_accessors(v, g, f"{(N, z0, nz)} {kind}")


def test_voxelized_grid_across_the_stride_boundary(v):
    """0 / 1 grids are what they were: the voxelizer's own output at 258^3"""
    v.Voxelize(258, frameIndex=0)
    g = v.Grid()
    assert g.any() and g.max() == 1
    check_accessors(v, g, "bunny 258")
    assert np.array_equal(v.GridBits(), np.packbits(g.reshape(-1), bitorder="little"))    # the wrapper's docstring, literally


# ---- the context's count and bit buffers under three frames ---------------------------------------------------------------------------
def test_three_frames_of_different_sizes_each_read_their_own(v, dxv):
    plan = [(0, (64, 0, 64)), (1, (10, 0, 7)), (2, (6, 1, 3))]
    grids = {}
    for frame, (N, z0, nz) in plan:
        v.Voxelize(N, 0, z0, nz, frameIndex=frame)
        grids[frame] = random_bytes(N * N * nz, 40 + frame).reshape(nz, N, N)
        write_grid(v, grids[frame])
    for order in ((0, 1, 0, 2, 0), (2, 1, 0, 1, 2), (1, 2, 0, 2, 1)):   # large, small, large; and the other way round
        for frame in order:
            v.SetFrame(frame)
            g = grids[frame]
            check_accessors(v, g, f"frame {frame} in {order}")
            nbytes = (g.size + 7) // 8
            room = np.full(nbytes + 64, 0xA5, np.uint8)                # exactly ceil(n / 8) bytes arrive, whatever the shared buffer holds
            got = v.GridBits(room[:nbytes])
            assert np.array_equal(got, np.packbits(g.reshape(-1) != 0, bitorder="little")) and (room[nbytes:] == 0xA5).all(), frame
            for wrong in (nbytes - 1, nbytes + 1, (grids[0].size + 7) // 8 if frame else 88):
                with pytest.raises(dxv.DxvError, match=f"expected {nbytes} bytes, got {wrong}"):
                    v.GridBits(np.empty(wrong, np.uint8))
    v.SetFrame(0)


# ---- checksum ----------------------------------------------------------------------------------------------------------------------
def checksum(v, ptr, nbytes):
    s = C.c_uint64(0xDEADBEEFDEADBEEF)
    rc = v._lib.dxv_scene_checksum(v._ctx, C.c_void_p(ptr) if ptr else None, nbytes, C.byref(s))
    return rc, s.value


WORDS = [1, 63, 64, 65, 255, 256, 257, 2048 * 256, 2048 * 256 + 1, 2 * 2048 * 256 + 77]     # one pass of k_checksum: 2048 x 256 words


@pytest.fixture(scope="module")
def random_words(dxvlib):
    """the largest buffer once: (host uint64 [max + 8], the same words on the device)"""
    import torch
    host = np.random.default_rng(99).integers(0, 2 ** 64, max(WORDS) + 8, dtype=np.uint64)      # full range: the sums wrap
    dev = torch.from_numpy(host).to("cuda")
    assert dev.dtype == torch.uint64
    torch.cuda.synchronize()
    return host, dev


@pytest.mark.parametrize("words", WORDS)
def test_checksum_equals_numpy_sum(v, random_words, words):
    _, dev = random_words
    back = dev.cpu().numpy()
    for first in (0, 1):                                                # the buffer's start, and a pointer 8 bytes into it
        want = int(back[first:first + words].sum(dtype=np.uint64))
        ptr = dev.data_ptr() + 8 * first
        for r in range(8):                                              # the trailing r bytes are no word: ignored
            rc, got = checksum(v, ptr, 8 * words + r)
            assert rc == 0 and got == want, (words, first, r, hex(got), hex(want))


def test_checksum_refuses_with_a_message_and_leaves_the_sum(v, random_words):
    _, dev = random_words
    for ptr, nbytes in ((dev.data_ptr(), 0), (dev.data_ptr(), 7), (0, 64), (0, 0)):
        rc, got = checksum(v, ptr, nbytes)
        assert rc == 1 and got == 0xDEADBEEFDEADBEEF, (ptr, nbytes)
        assert "dxv_scene_checksum: no blob" in v._lib.dxv_last_error(v._ctx).decode()
    rc, got = checksum(v, dev.data_ptr(), 8)
    assert rc == 0 and got == int(dev[:1].cpu().numpy()[0])


def test_checksum_of_an_exported_scene_equals_numpy_sum(v):
    import torch
    v.build_lists(parity=True, grid=64)                                 # the blob with both kinds of lists behind the tree
    nbytes = v.scene_bytes()
    blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    v.scene_export(blob.data_ptr(), nbytes)
    back = blob.cpu().numpy()
    want = int(back[:nbytes - nbytes % 8].view(np.uint64).sum(dtype=np.uint64))
    rc, got = checksum(v, blob.data_ptr(), nbytes)
    assert nbytes > 2048 * 256 * 8 and rc == 0 and got == want and got != 0, (nbytes, hex(got), hex(want))


# ---- the consumers agree -------------------------------------------------------------------------------------------------------------
def test_every_consumer_counts_the_same_solid_voxels(v, dxv):
    g = random_bytes(64 ** 3, 5).reshape(64, 64, 64)
    want = int(np.count_nonzero(g))
    v.Voxelize(64, frameIndex=0)
    write_grid(v, g)
    assert v.CountSolid() == want
    assert int(np.unpackbits(v.GridBits()).sum()) == want
    assert int((v.DistanceField(dxv.DIST_SQ_I32) < 0).sum()) == want
    v.Octree()
    v.OctreeExpand()
    back = v.Grid()
    assert int(np.count_nonzero(back)) == want and np.array_equal(back, (g != 0).astype(np.uint8))
    assert v.CountSolid() == want and int(np.unpackbits(v.GridBits()).sum()) == want
