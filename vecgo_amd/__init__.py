"""vecgo_amd — MI355X (gfx950) implementation of vecgo's distance + quantization hot path.

The product is libvecgo_hip.so (C ABI: include/vecgo_hip.h).  This package is the thin
Python binding the tests and bench.py drive it with; names mirror the reference's Go
interfaces (distance.Metric, quantization.ProductQuantizer, ...).
"""
from .api import (BinaryQuantizer, Comm, Context, Index, Int4Quantizer, Metric, OptimizedProductQuantizer, ProductQuantizer, RaBitQuantizer, ScalarQuantizer, Segment, VecgoHipError, crc32c, crc32c_device,  # noqa: F401
                  compact, compaction_plan, dot_batch, find_closest_centroids, hamming_batch, heap_replay, kmeans_assign, kmeans_train,
                  merge_indexes, merge_topk, merge_topk_packed, normalize_l2, pq_adc_lookup_batch, squared_l2_batch,
                  squared_l2_bounded_batch,
                  Columns, FilterOp, MaskOp, FILTER_CLAUSE, FILTER_TILE_ROWS, evaluate_filters, mask_combine, mask_popcount, pack_filter_sets,
                  mask_to_rows, MASK_ROWS_TILE_ROWS, PREFILTER_CHUNK_ROWS,
                  Bm25, BM25_TILE_DOCS, BM25_UPDATE_CHUNK, hybrid_search, rrf_fuse)

__all__ = ["BinaryQuantizer", "Comm", "Context", "Index", "Int4Quantizer", "Metric", "OptimizedProductQuantizer", "ProductQuantizer", "RaBitQuantizer", "ScalarQuantizer", "Segment", "VecgoHipError", "crc32c", "crc32c_device",
           "compact", "compaction_plan", "dot_batch", "find_closest_centroids", "hamming_batch", "heap_replay", "kmeans_assign", "kmeans_train",
           "merge_indexes", "merge_topk", "merge_topk_packed", "normalize_l2", "pq_adc_lookup_batch", "squared_l2_batch", "squared_l2_bounded_batch",
           "Columns", "FilterOp", "MaskOp", "FILTER_CLAUSE", "FILTER_TILE_ROWS", "evaluate_filters", "mask_combine", "mask_popcount", "pack_filter_sets",
           "mask_to_rows", "MASK_ROWS_TILE_ROWS", "PREFILTER_CHUNK_ROWS",
           "Bm25", "BM25_TILE_DOCS", "BM25_UPDATE_CHUNK", "hybrid_search", "rrf_fuse"]
