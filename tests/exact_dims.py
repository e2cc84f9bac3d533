"""How the exact fp32 scorers of vecgo_amd/csrc/vg_exact.hpp walk a row's 64-float blocks and its tail, restated in Python so that a
test can pick the dimensions at which every loop of every form runs and say which it reached.  No GPU.

  loops       exact_pair16 / exact_l2_both16 ("plain": kExactChunk blocks at a time, then kExactChunkSmall, then singles; "qlds", the
              query read from LDS: VG_QLDS_CHUNK, then kExactChunkSmall, then singles) and exact_rowregs16 / exact_rowregs16x2
              ("regs": up to 16 blocks held in registers, each a guarded step of one unrolled loop), with the tail of every mode:
              kBatch 16-wide steps then scalars, kBounded 8-wide steps then scalars, kPair (and the register forms) scalars only
  regs_form   thr_scan_regs (vg_search.hpp) and the flat small-batch scan's gate (flat_search_masked, k_flat.hip)
  brute_mq    the gate of brute_dist_mq_kernel (brute_impl, k_brute.hip); the grouped fp32 probe (k_probe.hip) has the same rule
  HNSW_LDS_EF kHnswLdsEf (k_graph.hip): the fp32 walk's heaps are split above it, and the split walk is the "qlds" form's only caller

tests/test_exact_dims_cpu.py holds these against the headers and DIMS against the classes the GPU tests are to reach."""
from collections import namedtuple

BLOCK = 64                                     # floats per block: one float4 per lane of the 16-lane group, four accumulators
EXACT_CHUNK, EXACT_CHUNK_SMALL, QLDS_CHUNK = 12, 4, 6
REGS_MAX_BLOCKS = 16
HNSW_LDS_EF = 512

FORMS = ("plain", "qlds", "regs")

# big / four / single: trips of the three block loops; blocks: dim // 64; tail: the floats behind the last block;
# batch16, batch_scalar: kBatch's 16-wide steps and the scalars after them; bounded8, bounded_scalar: kBounded's 8-wide steps and
# scalars; pair_scalar: kPair's scalar tail (all of it)
Loops = namedtuple("Loops", "big four single blocks tail batch16 batch_scalar bounded8 bounded_scalar pair_scalar")


def loops(dim, form):
    if form not in FORMS:
        raise ValueError(form)
    blocks, tail = dim // BLOCK, dim % BLOCK
    if form == "regs":
        if blocks > REGS_MAX_BLOCKS:
            raise ValueError(f"the register forms hold {REGS_MAX_BLOCKS} blocks, dim {dim} has {blocks}")
        big, four, single = 0, 0, blocks
    else:
        chunk = EXACT_CHUNK if form == "plain" else QLDS_CHUNK
        big, left = divmod(blocks, chunk)
        four, single = divmod(left, EXACT_CHUNK_SMALL)
    return Loops(big, four, single, blocks, tail, tail // 16, tail % 16, tail // 8, tail % 8, tail)


def trips(dim, form):
    """(big, four, single) of loops(dim, form)"""
    return tuple(loops(dim, form)[:3])


def regs_form(dim):
    """thr_scan_regs and the flat small-batch scan: rows of whole float4, at least one block, at most 16 (the rows are 16-byte
    aligned whenever dim % 4 == 0: the index allocates them)"""
    return dim % 4 == 0 and 64 <= dim <= 1024


def brute_mq(dim):
    """brute_dist_mq_kernel (two or more queries, a shared mask or none) and the grouped fp32 probe: no lower bound"""
    return dim % 4 == 0 and dim <= 1024


# The dimensions tests/test_gpu_exact_dims.py runs; tests/test_exact_dims_cpu.py lists the classes they have to cover.
#        blocks  tail   plain    qlds     what it is here for
#   60      0     60    (0,0,0)  (0,0,0)  just below regs_form's lower edge; brute_mq with no block at all
#  256      4      0    (0,1,0)  (0,1,0)  the 4-block loop alone
#  324      5      4    (0,1,1)  (0,1,1)
#  400      6     16    (0,1,2)  (1,0,0)  the QLDS chunk alone; one 16-wide step, two 8-wide steps, no scalar
#  455      7      7    (0,1,3)  (1,0,1)  odd: rows not 16-byte aligned
#  512      8      0    (0,2,0)  (1,0,2)
#  580      9      4    (0,2,1)  (1,0,3)
#  660     10     20    (0,2,2)  (1,1,0)  tail 16 + 4; kBounded 2 x 8 + 4 scalars
#  767     11     63    (0,2,3)  (1,1,1)  odd; the longest tail: 3 x 16 + 15, 7 x 8 + 7
#  832     13      0    (1,0,1)  (2,0,1)
# 1020     15     60    (1,0,3)  (2,0,3)  the last dim of 15 register blocks, a 60-float scalar tail
# 1024     16      0    (1,1,0)  (2,1,0)  the register forms' last dim
# 1028     16      4    (1,1,0)  (2,1,0)  just outside both register gates: the from-memory kernels
# 1100     17     12    (1,1,1)  (2,1,1)
# 1535     23     63    (1,2,3)  (3,1,1)  odd
# 1792     28      0    (2,1,0)  (4,1,0)
DIMS = [60, 256, 324, 400, 455, 512, 580, 660, 767, 832, 1020, 1024, 1028, 1100, 1535, 1792]
