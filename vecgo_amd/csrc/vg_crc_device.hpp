// vg_crc_device.hpp — the device CRC-32C of k_flat_build.hip for the segment writers (vg_segment_write_flat there,
// vg_segment_write_diskann in k_diskann_build.hip): the kernels and the definitions stay in k_flat_build.hip.
#pragma once

#include "vg_internal.hpp"

namespace vg {

struct CrcTables;  // slicing, skip and tail tables, one copy per device for the life of the process
int32_t crc_tables(int device, const CrcTables **out);

// One byte range's CRC in two steps: launch() enqueues the kernels, which leave head, tail and the blocks' registers in
// d_out[0 .. words()); finish() chains a host copy of them.
struct CrcJob {
    int64_t size = 0, head = 0, pieces = 0, tail = 0, blocks = 0;
    void plan(const void *ptr, int64_t bytes);
    size_t words() const { return static_cast<size_t>(blocks) + 2; }
    int32_t launch(const void *ptr, const CrcTables *tables, uint32_t *d_out, hipStream_t st) const;
    // the raw register of the whole range
    uint32_t finish(const uint32_t *h_out) const;
};

}  // namespace vg
