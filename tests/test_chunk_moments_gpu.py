"""GPU: chunk_moments_u8 (include/convnet_hip.h, csrc/dataset_moments.hip) through the C ABI and Matrix.ChunkMomentsU8.  Every sum is
an integer, so acc is compared with numpy's int64 sums for EQUALITY (tests/moments_ref.py: int_moments): both load paths of the kernel
(dword loads where the pixel count is a multiple of 4, byte loads elsewhere), an unaligned sub-range, the 32-bit overflow of a sum of
squares, accumulation, the error codes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from moments_ref import int_moments  # noqa: E402

ERR_INCOMPATIBLE, ERR_GENERIC, ERR_UNSUPPORTED = -1, -6, -9


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from convnet_amd.matrix import Matrix
    Matrix.SetupCUDADevice(0)
    return Matrix


def chunk_of(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).cuda()


def new_acc(dims, C, fill=0):
    import torch
    return torch.full((2 * dims + C * C,), fill, dtype=torch.int64, device="cuda")


def random_rows(C, H, W, cases, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (cases, C * H * W), dtype=np.uint8)


@pytest.mark.parametrize("C,H,W,cases", [(1, 28, 28, 3), (3, 8, 8, 5), (4, 4, 4, 1), (3, 5, 7, 9), (2, 3, 3, 300), (1, 40, 40, 3),
                                          (2, 17, 19, 4), (1, 512, 256, 37), (1, 181, 181, 37)])
def test_whole_chunk_is_bit_equal_to_int64_sums(gpu, C, H, W, cases):
    """The issue's three shapes; 105 dims (byte loads); 300 cases in 10 shares; 1 600 and 323 pixels: several tiles across the pixels,
    the last partly idle, on the dword and on the byte path; 131 072 and 32 761 pixels: 512 tiles, so the 37 cases are ONE share and a
    wave walks 9 or 10 of them (the unrolled loop and its remainder)."""
    rows = random_rows(C, H, W, cases, seed=C * 100 + cases)
    dims = C * H * W
    acc = new_acc(dims, C)
    gpu.ChunkMomentsU8(chunk_of(rows), dims, cases, 0, cases, C, acc)
    assert np.array_equal(acc.cpu().numpy(), int_moments(rows, C))


def test_unaligned_sub_range_leaves_the_neighbours_out(gpu):
    """dims = 105 is no multiple of 16 or 4: the range starts at byte 105, odd.  Cases 0 and 8 are not counted."""
    C, H, W, cases = 3, 5, 7, 9
    rows = random_rows(C, H, W, cases, seed=11)
    dims = C * H * W
    acc = new_acc(dims, C)
    gpu.ChunkMomentsU8(chunk_of(rows), dims, cases, 1, 7, C, acc)
    assert np.array_equal(acc.cpu().numpy(), int_moments(rows[1:8], C))
    assert not np.array_equal(acc.cpu().numpy(), int_moments(rows, C))


def test_dword_path_from_a_base_that_is_not_dword_aligned(gpu):
    """P = 64 pixels would take dword loads; a chunk that starts one byte into an allocation must not."""
    import torch
    C, H, W, cases = 3, 8, 8, 5
    rows = random_rows(C, H, W, cases, seed=12)
    dims = C * H * W
    store = torch.zeros(1 + rows.size, dtype=torch.uint8, device="cuda")
    chunk = store[1:]
    chunk.copy_(torch.from_numpy(rows.reshape(-1)))
    assert chunk.data_ptr() % 4 == 1
    acc = new_acc(dims, C)
    gpu.ChunkMomentsU8(chunk, dims, cases, 0, cases, C, acc)
    assert np.array_equal(acc.cpu().numpy(), int_moments(rows, C))


def test_sum_of_squares_crosses_32_bits(gpu):
    """70 000 cases of all-255 bytes: sum x^2 = 255^2 * 70 000 > 2^32 (it crosses at 66 052 cases); an 840 KB chunk."""
    C, H, W, cases = 3, 2, 2, 70000
    rows = np.full((cases, C * H * W), 255, np.uint8)
    dims = C * H * W
    acc = new_acc(dims, C)
    gpu.ChunkMomentsU8(chunk_of(rows), dims, cases, 0, cases, C, acc)
    got = acc.cpu().numpy()
    assert got[dims] == 255 * 255 * cases > 1 << 32
    assert np.array_equal(got, int_moments(rows, C))


def test_two_halves_add_up_to_the_whole_and_runs_repeat(gpu):
    C, H, W, cases = 3, 8, 8, 10
    rows = random_rows(C, H, W, cases, seed=13)
    dims = C * H * W
    chunk = chunk_of(rows)
    whole, halves, again = new_acc(dims, C), new_acc(dims, C), new_acc(dims, C)
    gpu.ChunkMomentsU8(chunk, dims, cases, 0, cases, C, whole)
    gpu.ChunkMomentsU8(chunk, dims, cases, 0, 5, C, halves)
    gpu.ChunkMomentsU8(chunk, dims, cases, 5, 5, C, halves)
    gpu.ChunkMomentsU8(chunk, dims, cases, 0, cases, C, again)
    assert np.array_equal(whole.cpu().numpy(), int_moments(rows, C))
    assert np.array_equal(halves.cpu().numpy(), whole.cpu().numpy())
    assert np.array_equal(again.cpu().numpy(), whole.cpu().numpy())          # the same call, the same bits


def test_the_entry_adds_and_zero_cases_write_nothing(gpu):
    C, H, W, cases = 3, 8, 8, 4
    rows = random_rows(C, H, W, cases, seed=14)
    dims = C * H * W
    acc = new_acc(dims, C, fill=7)
    gpu.ChunkMomentsU8(chunk_of(rows), dims, cases, 2, 0, C, acc)
    assert (acc.cpu().numpy() == 7).all()
    gpu.ChunkMomentsU8(chunk_of(rows), dims, cases, 0, cases, C, acc)
    assert np.array_equal(acc.cpu().numpy(), int_moments(rows, C) + 7)


def test_error_codes(gpu):
    from convnet_amd._lib import lib
    C, H, W, cases = 3, 4, 4, 6
    rows = random_rows(C, H, W, cases, seed=15)
    dims = C * H * W
    chunk, acc = chunk_of(rows), new_acc(dims, 5, fill=3)      # (room for the 5-colour call below)
    c, a = ctypes.c_void_p(chunk.data_ptr()), ctypes.c_void_p(acc.data_ptr())
    assert lib.chunk_moments_u8(None, dims, cases, 0, cases, C, a) == ERR_GENERIC
    assert lib.chunk_moments_u8(c, dims, cases, 0, cases, C, None) == ERR_GENERIC
    assert lib.chunk_moments_u8(c, dims, cases, 0, cases, 5, a) == ERR_INCOMPATIBLE          # 48 % 5 != 0
    assert lib.chunk_moments_u8(c, dims, cases, 0, -1, C, a) == ERR_INCOMPATIBLE
    assert lib.chunk_moments_u8(c, dims, cases, 2, cases - 1, C, a) == ERR_INCOMPATIBLE      # ends behind the chunk
    assert lib.chunk_moments_u8(c, dims, cases, -1, 2, C, a) == ERR_INCOMPATIBLE
    assert lib.chunk_moments_u8(c, dims, cases, cases + 1, 0, C, a) == ERR_INCOMPATIBLE
    assert lib.chunk_moments_u8(c, 40, 7, 0, 7, 5, a) == ERR_UNSUPPORTED                     # 5 colours: the host's matrix path
    assert lib.chunk_moments_u8(c, dims, cases, cases, 0, C, a) == 0                         # an empty range at the very end
    import torch
    torch.cuda.synchronize()
    assert (acc.cpu().numpy() == 3).all()                                                    # none of them wrote
