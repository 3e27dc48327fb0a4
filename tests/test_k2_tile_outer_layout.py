"""What the tile-outer K2 (csrc/mlp_k2_f16x1_to.hip) takes for granted about the precision-4/5 surface blob, held against the header the packer writes
(csrc/pack_blob.hip through nerfart_pack_plan_debug: integer work, no GPU).  The kernel numbers a layer's first chunk itself (to_first_chunk) and
addresses item (k-step u, tile T) of a layer at that chunk's offset + (16 u + T) * 512 floats, i.e. it needs a layer's chunks back to back."""
import ctypes as C
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = 16 * 512                       # floats of one k-step: 16 output tiles x (hi, lo) fragments of 1 KiB each
K_STEPS = [2, 8, 8, 8, 9, 8, 8, 8]  # layer 0: two encoding units; the skip layer: 7 hidden units + 2 encoding units


def to_first_chunk(l):              # the kernel's own formula, csrc/mlp_k2_f16x1_to.hip
    return 0 if l == 0 else (4 * l - 3 if l <= 4 else 4 * l - 2)


def _header(fp16):
    lib = C.CDLL(os.path.join(REPO, "nerfart_amd", "csrc", "libnerfart_hip.so"))
    lib.nerfart_pack_plan_debug.restype = C.c_int
    lib.nerfart_pack_plan_debug.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    sizes = (C.c_longlong * 4)()
    assert lib.nerfart_pack_plan_debug(3, 1, fp16, sizes, None, None, None, None, None) == 0
    n_c, n_a = int(sizes[0]), int(sizes[1])
    hdr = np.zeros(512, np.int32); ci = np.zeros(n_c, np.int32); cm = np.zeros(n_c, np.int32); cs = np.zeros(n_c, np.float32); ai = np.zeros(n_a, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.nerfart_pack_plan_debug(3, 1, fp16, sizes, p(hdr), p(ci), p(cm), p(cs), p(ai)) == 0
    return hdr


@pytest.mark.parametrize("fp16", [1, 2])            # precision 4's blob, precision 5's (the scaled recursion: same layout, another encoding word)
def test_layer_chunks_are_numbered_and_contiguous_as_the_kernel_assumes(fp16):
    hdr = _header(fp16)
    offs = hdr[16:16 + 31].astype(np.int64)
    assert int(hdr[2]) == 30, "chunks of the forward program"
    c = 0
    for l, nks in enumerate(K_STEPS):
        assert to_first_chunk(l) == c, f"layer {l} starts at chunk {c}"
        n_chunks = (nks + 1) // 2
        for k in range(n_chunks + 1):
            # chunk k of the layer holds its k-steps 2k, 2k + 1: item (u, T) at tab[u / 2] + ((u & 1) * 16 + T) * 512 = the layer's first offset + (16 u + T) * 512
            assert offs[c + k] == offs[c] + min(2 * k, nks) * KS, (l, k)
        c += n_chunks
    assert c == 30 and offs[30] - offs[0] == sum(K_STEPS) * KS
