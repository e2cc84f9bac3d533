// vecgo_hip.hpp — C++ host-side mirror of the reference's Go interfaces over the C ABI.
//
// The reference is compiled Go; no Go toolchain exists in the build image, so the host side
// above the C ABI is C++ (header-only, no dependency beyond vecgo_hip.h).  Names, argument
// meaning and error behaviour follow the reference:
//   vecgo::distance::Metric / Provider           distance/distance.go:66-116
//   vecgo::quantization::Quantizer               internal/quantization/quantizer.go:12-24
//   vecgo::quantization::ProductQuantizer        internal/quantization/pq.go:20-500
//   vecgo::quantization::RaBitQuantizer          internal/quantization/rabitq.go:26-190
//   vecgo::kmeans::TrainKMeans / AssignPartition internal/kmeans/kmeans.go:16-280
//   vecgo::Segment                               flat.Segment.Search / Rerank, hnsw.KNNSearch,
//                                                diskann searchInternal (one query batch per call)
// Go's (value, error) becomes a thrown vecgo::Error carrying the Go error string.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vecgo_hip.h"

namespace vecgo {

class Error : public std::runtime_error {
public:
    Error(int32_t status, const std::string &msg) : std::runtime_error(msg), status_(status) {}
    int32_t status() const { return status_; }

private:
    int32_t status_;
};

inline void check(int32_t status)
{
    if (status == VG_OK) return;
    const char *m = vg_last_error();
    throw Error(status, (m && *m) ? m : vg_status_string(status));
}

// One per (process, GPU).
class Context {
public:
    explicit Context(int device = 0) { check(vg_ctx_create(device, &h_)); }
    ~Context() { vg_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    vg_ctx *handle() const { return h_; }

private:
    vg_ctx *h_ = nullptr;
};

namespace distance {

// distance.Metric (distance/distance.go:66-73)
enum class Metric : int32_t { L2 = VG_METRIC_L2, Cosine = VG_METRIC_COSINE, Dot = VG_METRIC_DOT, Hamming = VG_METRIC_HAMMING };

// Metric.String (distance/distance.go:75-88), "Unknown(%d)" for anything else.  (Returns std::string since r04, when
// the "Unknown(%d)" form was added — a source break for `const char *s = String(m)`; CString keeps the C-string form
// for the four named metrics and says "Unknown" for the rest.)
inline const char *CString(Metric m)
{
    switch (m) {
    case Metric::L2: return "L2";
    case Metric::Cosine: return "Cosine";
    case Metric::Dot: return "Dot";
    case Metric::Hamming: return "Hamming";
    }
    return "Unknown";
}
inline std::string String(Metric m)
{
    switch (m) {
    case Metric::L2: return "L2";
    case Metric::Cosine: return "Cosine";
    case Metric::Dot: return "Dot";
    case Metric::Hamming: return "Hamming";
    }
    return "Unknown(" + std::to_string(static_cast<int32_t>(m)) + ")";
}

// distance.Func is a single-pair function in the reference; on the GPU the unit is one query
// against n contiguous targets (simd.SquaredL2Batch / DotBatch, internal/simd/kernels.go:61-68).
using BatchFunc = void (*)(const Context &, const float *query, const float *targets, int64_t dim, int64_t n, float *out);

inline void SquaredL2Batch(const Context &c, const float *q, const float *t, int64_t dim, int64_t n, float *out)
{
    check(vg_squared_l2_batch(c.handle(), q, t, dim, n, out, nullptr));
}
inline void DotBatch(const Context &c, const float *q, const float *t, int64_t dim, int64_t n, float *out)
{
    check(vg_dot_batch(c.handle(), q, t, dim, n, out, nullptr));
}

// distance.NormalizeL2InPlace (distance/distance.go:40-53): false for an empty or zero-norm vector (left untouched)
inline bool NormalizeL2InPlace(const Context &c, std::vector<float> &v)
{
    if (v.empty()) return false;
    uint8_t ok = 0;
    check(vg_normalize_l2(c.handle(), v.data(), 1, static_cast<int32_t>(v.size()), &ok, nullptr));
    return ok != 0;
}

// distance.Provider (distance/distance.go:91-106)
inline BatchFunc Provider(Metric m)
{
    switch (m) {
    case Metric::L2: return SquaredL2Batch;
    case Metric::Cosine:
    case Metric::Dot: return DotBatch;
    default: throw Error(VG_ERR_UNSUPPORTED, std::string("unsupported metric for float32: ") + String(m));
    }
}

}  // namespace distance

namespace quantization {

// quantization.Quantizer (internal/quantization/quantizer.go:12-24)
class Quantizer {
public:
    virtual ~Quantizer() = default;
    virtual std::vector<uint8_t> Encode(const std::vector<float> &v) = 0;
    virtual std::vector<float> Decode(const std::vector<uint8_t> &b) = 0;
    virtual void Train(const std::vector<std::vector<float>> &vectors) = 0;
    virtual int BytesPerDimension() const = 0;
};

// quantization.ProductQuantizer (pq.go:20-29)
class ProductQuantizer : public Quantizer {
public:
    // NewProductQuantizer (pq.go:36-64)
    ProductQuantizer(std::shared_ptr<Context> ctx, int dimension, int numSubvectors, int numCentroids)
        : ctx_(std::move(ctx)), dim_(dimension), m_(numSubvectors), k_(numCentroids)
    {
        check(vg_pq_create(ctx_->handle(), dimension, numSubvectors, numCentroids, &h_));
    }
    ~ProductQuantizer() override { vg_pq_destroy(h_); }
    vg_pq *handle() const { return h_; }

    // Train (pq.go:68-143); the reference runs 20 Lloyd iterations
    void Train(const std::vector<std::vector<float>> &vectors) override
    {
        if (vectors.empty()) throw Error(VG_ERR_INVALID_ARG, "no vectors provided for training");
        if (static_cast<int>(vectors[0].size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<float> flat;
        flat.reserve(vectors.size() * static_cast<size_t>(dim_));
        for (const auto &v : vectors) flat.insert(flat.end(), v.begin(), v.end());
        TrainFlat(flat.data(), static_cast<int64_t>(vectors.size()), 20, seed_);
    }
    void TrainFlat(const float *vectors, int64_t n, int iters, uint64_t seed)
    {
        check(vg_pq_train(h_, vectors, n, iters, seed, nullptr));
    }
    void SetSeed(uint64_t seed) { seed_ = seed; }

    // Encode (pq.go:147-176)
    std::vector<uint8_t> Encode(const std::vector<float> &vec) override
    {
        if (!IsTrained()) throw Error(VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
        if (static_cast<int>(vec.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint8_t> codes(static_cast<size_t>(m_));
        check(vg_pq_encode(h_, vec.data(), 1, codes.data(), nullptr));
        return codes;
    }
    void EncodeBatch(const float *vectors, int64_t n, uint8_t *codes) { check(vg_pq_encode(h_, vectors, n, codes, nullptr)); }

    // Decode (pq.go:185-229)
    std::vector<float> Decode(const std::vector<uint8_t> &codes) override
    {
        if (!IsTrained()) throw Error(VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
        if (static_cast<int>(codes.size()) != m_) throw Error(VG_ERR_CODE_LENGTH, "invalid code length");
        std::vector<float> out(static_cast<size_t>(dim_));
        check(vg_pq_decode(h_, codes.data(), 1, out.data(), nullptr));
        return out;
    }

    // ComputeAsymmetricDistance (pq.go:234-260)
    float ComputeAsymmetricDistance(const std::vector<float> &query, const std::vector<uint8_t> &codes)
    {
        if (!IsTrained()) throw Error(VG_ERR_NOT_TRAINED, "ProductQuantizer not trained");
        float d = 0.0f;
        check(vg_pq_asymmetric_distance_batch(h_, query.data(), codes.data(), 1, &d, nullptr));
        return d;
    }

    // BuildDistanceTable (pq.go:468-491) / AdcDistance (pq.go:495-500)
    std::vector<float> BuildDistanceTable(const std::vector<float> &query)
    {
        if (static_cast<int>(query.size()) != dim_)
            throw Error(VG_ERR_DIM_MISMATCH, "query dimension mismatch: expected " + std::to_string(dim_) + ", got " +
                                                 std::to_string(query.size()));
        std::vector<float> table(static_cast<size_t>(m_) * k_);
        check(vg_pq_build_distance_table(h_, query.data(), 1, table.data(), nullptr));
        return table;
    }
    float AdcDistance(const std::vector<float> &table, const std::vector<uint8_t> &codes)
    {
        if (static_cast<int>(codes.size()) != m_) throw Error(VG_ERR_CODE_LENGTH, "codes length mismatch");
        float d = 0.0f;
        check(vg_pq_adc_lookup_batch(ctx_->handle(), table.data(), codes.data(), m_, 1, &d, nullptr));
        return d;
    }

    // Codebooks / SetCodebooks (pq.go:452-464)
    void SetCodebooks(const std::vector<int8_t> &codebooks, const std::vector<float> &scales, const std::vector<float> &offsets)
    {
        check(vg_pq_set_codebooks(h_, codebooks.data(), scales.data(), offsets.data()));
    }
    void Codebooks(std::vector<int8_t> &codebooks, std::vector<float> &scales, std::vector<float> &offsets)
    {
        codebooks.resize(static_cast<size_t>(m_) * k_ * (dim_ / m_));
        scales.resize(static_cast<size_t>(m_));
        offsets.resize(static_cast<size_t>(m_));
        check(vg_pq_get_codebooks(h_, codebooks.data(), scales.data(), offsets.data()));
    }

    int BytesPerDimension() const override { return 0; }
    int BytesPerVector() const { return m_; }                                         // pq.go:263-265
    double CompressionRatio() const { return static_cast<double>(dim_) * 4.0 / m_; }  // pq.go:268-272
    int NumSubvectors() const { return m_; }
    int NumCentroids() const { return k_; }
    bool IsTrained() const { return vg_pq_is_trained(h_) != 0; }

private:
    std::shared_ptr<Context> ctx_;
    vg_pq *h_ = nullptr;
    int dim_, m_, k_;
    uint64_t seed_ = 1;
};

// quantization.RaBitQuantizer (rabitq.go:26-49)
class RaBitQuantizer : public Quantizer {
public:
    RaBitQuantizer(std::shared_ptr<Context> ctx, int dimension) : ctx_(std::move(ctx)), dim_(dimension) {}
    std::vector<uint8_t> Encode(const std::vector<float> &v) override
    {
        if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint8_t> out(static_cast<size_t>(BytesTotal()));
        check(vg_rabitq_encode(ctx_->handle(), dim_, v.data(), 1, out.data(), nullptr));
        return out;
    }
    std::vector<float> Decode(const std::vector<uint8_t> &) override
    {
        throw Error(VG_ERR_UNSUPPORTED, "RaBitQuantizer.Decode is not on the hot path");
    }
    void Train(const std::vector<std::vector<float>> &) override {}  // rabitq.go:179-181: no-op
    // Distance (rabitq.go:119-176)
    float Distance(const std::vector<float> &query, const std::vector<uint8_t> &code)
    {
        if (static_cast<int64_t>(code.size()) < BytesTotal()) throw Error(VG_ERR_CODE_LENGTH, "invalid code length");
        float d = 0.0f;
        check(vg_rabitq_distance_batch(ctx_->handle(), dim_, query.data(), code.data(), 1, &d, nullptr));
        return d;
    }
    int BytesPerDimension() const override { return 0; }                   // rabitq.go:183-185
    int64_t BytesTotal() const { return vg_rabitq_code_bytes(dim_); }      // rabitq.go:187-190

private:
    std::shared_ptr<Context> ctx_;
    int dim_;
};

// quantization.BinaryQuantizer (binary.go:23-262)
class BinaryQuantizer : public Quantizer {
public:
    BinaryQuantizer(std::shared_ptr<Context> ctx, int dimension) : ctx_(std::move(ctx)), dim_(dimension) {}
    BinaryQuantizer &WithThreshold(float t)  // binary.go:52-56
    {
        threshold_ = t;
        trained_ = true;
        return *this;
    }
    void Train(const std::vector<std::vector<float>> &vectors) override  // binary.go:59-79
    {
        if (vectors.empty()) throw Error(VG_ERR_INVALID_ARG, "no vectors provided for training");
        std::vector<float> flat;
        for (const auto &v : vectors) flat.insert(flat.end(), v.begin(), v.end());
        check(vg_binary_train(ctx_->handle(), dim_, flat.data(), static_cast<int64_t>(vectors.size()), &threshold_, nullptr));
        trained_ = true;
    }
    std::vector<uint8_t> Encode(const std::vector<float> &v) override  // binary.go:86-115 (= EncodeUint64's words)
    {
        if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint8_t> out(static_cast<size_t>(vg_binary_code_bytes(dim_)));
        check(vg_binary_encode(ctx_->handle(), dim_, threshold_, v.data(), 1, out.data(), nullptr));
        return out;
    }
    std::vector<uint64_t> EncodeUint64(const std::vector<float> &v)  // binary.go:118-154
    {
        const auto bytes = Encode(v);
        std::vector<uint64_t> words(bytes.size() / 8);
        std::memcpy(words.data(), bytes.data(), bytes.size());
        return words;
    }
    std::vector<float> Decode(const std::vector<uint8_t> &b) override  // binary.go:173-188
    {
        std::vector<float> out(static_cast<size_t>(dim_));
        check(vg_binary_decode(ctx_->handle(), dim_, threshold_, b.data(), 1, static_cast<int32_t>(b.size()), out.data(), nullptr));
        return out;
    }
    int ComputeHammingDistance(const std::vector<float> &query, const std::vector<uint64_t> &codes)  // binary.go:158-171
    {
        if (static_cast<int>(query.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint64_t> padded(static_cast<size_t>((dim_ + 63) / 64), 0);  // HammingDistance truncates to the shorter
        std::memcpy(padded.data(), codes.data(), std::min(codes.size(), padded.size()) * 8);
        int32_t d = 0;
        check(vg_binary_hamming_batch(ctx_->handle(), dim_, threshold_, query.data(),
                                      reinterpret_cast<const uint8_t *>(padded.data()), 1, &d, nullptr));
        return d;
    }
    int BytesPerDimension() const override { return 0; }     // binary.go:193-195
    int BytesTotal() const { return (dim_ + 7) / 8; }        // binary.go:198-200
    float Threshold() const { return threshold_; }
    bool IsTrained() const { return trained_; }
    float CompressionRatio() const { return 32.0f; }

private:
    std::shared_ptr<Context> ctx_;
    int dim_;
    float threshold_ = 0.0f;
    bool trained_ = false;
};

// quantization.OptimizedProductQuantizer (opq.go:15-307)
class OptimizedProductQuantizer : public Quantizer {
public:
    OptimizedProductQuantizer(std::shared_ptr<Context> ctx, int dimension, int numSubvectors, int numCentroids, int numIterations)
        : ctx_(std::move(ctx)), dim_(dimension), m_(numSubvectors)
    {
        check(vg_opq_create(ctx_->handle(), dimension, numSubvectors, numCentroids, numIterations, &h_));
    }
    ~OptimizedProductQuantizer() override { vg_opq_destroy(h_); }
    OptimizedProductQuantizer(const OptimizedProductQuantizer &) = delete;
    OptimizedProductQuantizer &operator=(const OptimizedProductQuantizer &) = delete;
    void Train(const std::vector<std::vector<float>> &vectors) override  // opq.go:89-193
    {
        if (vectors.empty()) throw Error(VG_ERR_INVALID_ARG, "no vectors provided for training");
        if (static_cast<int>(vectors[0].size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<float> flat;
        for (const auto &v : vectors) flat.insert(flat.end(), v.begin(), v.end());
        check(vg_opq_train(h_, flat.data(), static_cast<int64_t>(vectors.size()), 20, 1, nullptr));
    }
    std::vector<uint8_t> Encode(const std::vector<float> &v) override  // opq.go:218-231
    {
        if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint8_t> out(static_cast<size_t>(m_));
        check(vg_opq_encode(h_, v.data(), 1, out.data(), nullptr));
        return out;
    }
    std::vector<float> Decode(const std::vector<uint8_t> &b) override  // opq.go:234-269
    {
        if (static_cast<int>(b.size()) != m_) throw Error(VG_ERR_CODE_LENGTH, "invalid code length");
        std::vector<float> out(static_cast<size_t>(dim_));
        check(vg_opq_decode(h_, b.data(), 1, out.data(), nullptr));
        return out;
    }
    float ComputeAsymmetricDistance(const std::vector<float> &query, const std::vector<uint8_t> &codes)  // opq.go:272-286
    {
        float d = 0.0f;
        check(vg_opq_asymmetric_distance_batch(h_, query.data(), codes.data(), 1, &d, nullptr));
        return d;
    }
    std::vector<float> Rotations(int &blockSize, int &numBlocks) const
    {
        int32_t b = 0, nb = 0;
        check(vg_opq_get_rotations(h_, &b, &nb, nullptr));
        std::vector<float> r(static_cast<size_t>(nb) * b * b);
        check(vg_opq_get_rotations(h_, nullptr, nullptr, r.data()));
        blockSize = b;
        numBlocks = nb;
        return r;
    }
    int BytesPerDimension() const override { return 0; }
    int BytesPerVector() const { return m_; }                               // opq.go:289-291
    double CompressionRatio() const { return double(dim_) * 4.0 / m_; }     // opq.go:294-296
    bool IsTrained() const { return vg_opq_is_trained(h_) != 0; }

private:
    std::shared_ptr<Context> ctx_;
    vg_opq *h_ = nullptr;
    int dim_, m_;
};

// quantization.ScalarQuantizer (quantizer.go:27-39)
class ScalarQuantizer : public Quantizer {
public:
    // NewScalarQuantizer (quantizer.go:119-125)
    ScalarQuantizer(std::shared_ptr<Context> ctx, int dimension) : ctx_(std::move(ctx)), dim_(dimension)
    {
        check(vg_sq8_create(ctx_->handle(), dimension, &h_));
    }
    ~ScalarQuantizer() override { vg_sq8_destroy(h_); }
    vg_sq8 *handle() const { return h_; }
    bool IsTrained() const { return vg_sq8_is_trained(h_) != 0; }

    // Train (quantizer.go:127-180)
    void Train(const std::vector<std::vector<float>> &vectors) override
    {
        if (vectors.empty()) throw Error(VG_ERR_INVALID_ARG, "no vectors provided for training");
        if (static_cast<int>(vectors[0].size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<float> flat;
        flat.reserve(vectors.size() * static_cast<size_t>(dim_));
        for (const auto &v : vectors) {
            if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "inconsistent vector dimension");
            flat.insert(flat.end(), v.begin(), v.end());
        }
        check(vg_sq8_train(h_, flat.data(), static_cast<int64_t>(vectors.size()), nullptr));
    }
    // SetBounds (quantizer.go:52-78)
    void SetBounds(const std::vector<float> &mins, const std::vector<float> &maxs)
    {
        if (static_cast<int>(mins.size()) != dim_ || static_cast<int>(maxs.size()) != dim_)
            throw Error(VG_ERR_DIM_MISMATCH, "dimension mismatch");
        check(vg_sq8_set_bounds(h_, mins.data(), maxs.data()));
    }
    std::vector<float> Mins() const
    {
        std::vector<float> v(static_cast<size_t>(dim_));
        check(vg_sq8_get_params(h_, v.data(), nullptr, nullptr, nullptr));
        return v;
    }
    std::vector<float> Maxs() const
    {
        std::vector<float> v(static_cast<size_t>(dim_));
        check(vg_sq8_get_params(h_, nullptr, v.data(), nullptr, nullptr));
        return v;
    }
    // Encode / Decode (quantizer.go:183-250)
    std::vector<uint8_t> Encode(const std::vector<float> &v) override
    {
        if (!IsTrained()) throw Error(VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
        if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<uint8_t> out(static_cast<size_t>(dim_));
        check(vg_sq8_encode(h_, v.data(), 1, out.data(), nullptr));
        return out;
    }
    std::vector<float> Decode(const std::vector<uint8_t> &b) override
    {
        if (!IsTrained()) throw Error(VG_ERR_NOT_TRAINED, "ScalarQuantizer not trained");
        if (static_cast<int>(b.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "vector dimension mismatch");
        std::vector<float> out(static_cast<size_t>(dim_));
        check(vg_sq8_decode(h_, b.data(), 1, out.data(), nullptr));
        return out;
    }
    // L2DistanceBatch (quantizer.go:93-106)
    void L2DistanceBatch(const std::vector<float> &q, const std::vector<uint8_t> &codes, int n, std::vector<float> &out)
    {
        if (static_cast<int>(q.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "query dimension mismatch");
        if (static_cast<int64_t>(codes.size()) < static_cast<int64_t>(n) * dim_)
            throw Error(VG_ERR_INVALID_ARG, "codes buffer too small");
        if (static_cast<int>(out.size()) < n) throw Error(VG_ERR_INVALID_ARG, "output buffer too small");
        check(vg_sq8_l2_distance_batch(h_, q.data(), codes.data(), n, out.data(), nullptr));
    }
    int BytesPerDimension() const override { return 1; }
    double CompressionRatio() const { return 4.0; }

private:
    std::shared_ptr<Context> ctx_;
    int dim_;
    vg_sq8 *h_ = nullptr;
};

// quantization.Int4Quantizer (int4.go:12-20)
class Int4Quantizer : public Quantizer {
public:
    Int4Quantizer(std::shared_ptr<Context> ctx, int dimension) : ctx_(std::move(ctx)), dim_(dimension)
    {
        check(vg_int4_create(ctx_->handle(), dimension, &h_));
    }
    ~Int4Quantizer() override { vg_int4_destroy(h_); }
    vg_int4 *handle() const { return h_; }
    bool IsTrained() const { return vg_int4_is_trained(h_) != 0; }

    // Train (int4.go:29-62)
    void Train(const std::vector<std::vector<float>> &vectors) override
    {
        if (vectors.empty()) throw Error(VG_ERR_INVALID_ARG, "no vectors provided for training");
        std::vector<float> flat;
        flat.reserve(vectors.size() * static_cast<size_t>(dim_));
        for (const auto &v : vectors) {
            if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "dimension mismatch");
            flat.insert(flat.end(), v.begin(), v.end());
        }
        check(vg_int4_train(h_, flat.data(), static_cast<int64_t>(vectors.size()), nullptr));
    }
    // UnmarshalBinary (int4.go:190-219): min[dim] then diff[dim]
    void SetParams(const std::vector<float> &minVal, const std::vector<float> &diff)
    {
        if (static_cast<int>(minVal.size()) != dim_ || static_cast<int>(diff.size()) != dim_)
            throw Error(VG_ERR_DIM_MISMATCH, "data size mismatch");
        check(vg_int4_set_params(h_, minVal.data(), diff.data()));
    }
    // Encode / Decode (int4.go:65-130)
    std::vector<uint8_t> Encode(const std::vector<float> &v) override
    {
        if (static_cast<int>(v.size()) != dim_) throw Error(VG_ERR_DIM_MISMATCH, "dimension mismatch");
        std::vector<uint8_t> out(static_cast<size_t>((dim_ + 1) / 2));
        check(vg_int4_encode(h_, v.data(), 1, out.data(), nullptr));
        return out;
    }
    std::vector<float> Decode(const std::vector<uint8_t> &b) override
    {
        if (static_cast<int>(b.size()) != (dim_ + 1) / 2) throw Error(VG_ERR_DIM_MISMATCH, "dimension mismatch");
        std::vector<float> out(static_cast<size_t>(dim_));
        check(vg_int4_decode(h_, b.data(), 1, out.data(), nullptr));
        return out;
    }
    // L2Distance (int4.go:133-147: lookup-table kernel) / L2DistanceBatch (int4.go:150-164)
    float L2Distance(const std::vector<float> &query, const std::vector<uint8_t> &code)
    {
        if (static_cast<int>(query.size()) != dim_ || static_cast<int>(code.size()) != (dim_ + 1) / 2)
            throw Error(VG_ERR_DIM_MISMATCH, "dimension mismatch");
        float d = 0.0f;
        check(vg_int4_l2_distance_batch(h_, query.data(), code.data(), 1, 1, &d, nullptr));
        return d;
    }
    void L2DistanceBatch(const std::vector<float> &query, const std::vector<uint8_t> &codes, int n, std::vector<float> &out)
    {
        if (static_cast<int64_t>(codes.size()) < static_cast<int64_t>(n) * ((dim_ + 1) / 2))
            throw Error(VG_ERR_INVALID_ARG, "codes buffer too small");
        if (static_cast<int>(out.size()) < n) throw Error(VG_ERR_INVALID_ARG, "output buffer too small");
        check(vg_int4_l2_distance_batch(h_, query.data(), codes.data(), n, 0, out.data(), nullptr));
    }
    int BytesPerDimension() const override { return 0; }  // sub-byte (int4.go:167-169)

private:
    std::shared_ptr<Context> ctx_;
    int dim_;
    vg_int4 *h_ = nullptr;
};

}  // namespace quantization

namespace kmeans {

// TrainKMeans (kmeans.go:16-138): empty result when n < k (the reference returns (nil, nil))
inline std::vector<float> TrainKMeans(const Context &c, const std::vector<float> &vectors, int dim, int k,
                                      distance::Metric metric, int maxIter, uint64_t seed = 1)
{
    std::vector<float> cent(static_cast<size_t>(k) * dim);
    int32_t produced = 0;
    check(vg_kmeans_train(c.handle(), vectors.data(), static_cast<int64_t>(vectors.size() / dim), dim, k,
                          static_cast<int32_t>(metric), maxIter, seed, cent.data(), &produced, nullptr));
    if (!produced) cent.clear();
    return cent;
}

// AssignPartition (kmeans.go:142-196)
inline int AssignPartition(const Context &c, const std::vector<float> &vec, const std::vector<float> &centroids, int dim,
                           distance::Metric metric)
{
    int32_t out = -1;
    check(vg_kmeans_assign(c.handle(), vec.data(), 1, dim, centroids.data(), static_cast<int32_t>(centroids.size() / dim),
                           static_cast<int32_t>(metric), &out, nullptr));
    return out;
}

// FindClosestCentroids (kmeans.go:217-280)
inline std::vector<int> FindClosestCentroids(const Context &c, const std::vector<float> &query,
                                             const std::vector<float> &centroids, int dim, int n, distance::Metric metric)
{
    const int k = static_cast<int>(centroids.size() / dim);
    std::vector<int32_t> out(static_cast<size_t>(std::max(1, std::min(n, k))));
    int32_t cnt = 0;
    check(vg_find_closest_centroids(c.handle(), query.data(), centroids.data(), dim, k, n, static_cast<int32_t>(metric),
                                    out.data(), &cnt, nullptr));
    return std::vector<int>(out.begin(), out.begin() + cnt);
}

}  // namespace kmeans

// hash.CRC32C (internal/hash/crc32c.go:15-17) of `size` bytes of device memory, computed on the device
inline uint32_t CRC32CDevice(const Context &c, const void *devicePtr, int64_t size)
{
    uint32_t out = 0;
    check(vg_crc32c_device(c.handle(), devicePtr, size, &out, nullptr));
    return out;
}

struct Result {
    std::vector<uint32_t> ids;   // [nq * k], best first, VG_INVALID_ID padded
    std::vector<float> scores;   // [nq * k]
};
// Engine.SearchThreshold's answer: per query counts[q] rows within the threshold, best first (at most max_results)
struct ThresholdResult {
    std::vector<uint32_t> ids;     // [nq * max_results], VG_INVALID_ID after counts[q]
    std::vector<float> scores;     // [nq * max_results]
    std::vector<int32_t> counts;   // [nq]
};

// One resident segment (flat / memtable-HNSW / DiskANN): the batch-level search entry points.
class Segment {
public:
    Segment(std::shared_ptr<Context> ctx, int64_t rows, int dim, distance::Metric metric)
        : ctx_(std::move(ctx)), n_(rows), dim_(dim)
    {
        check(vg_index_create(ctx_->handle(), rows, dim, static_cast<int32_t>(metric), &h_));
    }
    ~Segment() { vg_index_destroy(h_); }
    Segment(const Segment &) = delete;
    Segment &operator=(const Segment &) = delete;

    void SetVectors(const float *base) { check(vg_index_set_vectors(h_, base, nullptr)); }
    void SetPQCodes(std::shared_ptr<quantization::ProductQuantizer> pq, const uint8_t *codes)
    {
        pq_ = std::move(pq);
        check(vg_index_set_pq_codes(h_, pq_->handle(), codes, nullptr));
    }
    void SetRaBitQCodes(const uint8_t *codes) { check(vg_index_set_rabitq_codes(h_, codes, nullptr)); }
    void SetVamanaGraph(int r, const uint32_t *graph, uint32_t entry) { check(vg_index_set_vamana_graph(h_, r, graph, entry, nullptr)); }
    void SetHNSWLayer0(int m0, const uint32_t *l0, uint32_t entry)
    {
        check(vg_index_set_hnsw_graph(h_, m0, l0, 0, m0 / 2 > 0 ? m0 / 2 : 1, nullptr, nullptr, nullptr, entry, nullptr));
    }

    // flat.Segment.Search fp32 branch (flat/segment.go:691-721)
    Result SearchFlat(const float *queries, int64_t nq, int k) { return run(nq, k, [&](Result &r) { return vg_search_flat(h_, queries, nq, k, r.ids.data(), r.scores.data(), nullptr); }); }
    // Engine.SearchThreshold's flat-segment leg (engine/engine.go:1485-1531): Search(q, max_results), then the rows within
    // thresholds[q] (<= for L2, >= for Dot / Cosine); mask: the row filter of vg_search_flat_filtered (nullptr = none)
    ThresholdResult SearchThreshold(const float *queries, int64_t nq, const float *thresholds, int max_results,
                                    const uint8_t *mask = nullptr, int64_t mask_stride = 0)
    {
        ThresholdResult r;
        r.ids.resize(static_cast<size_t>(nq) * max_results);
        r.scores.resize(static_cast<size_t>(nq) * max_results);
        r.counts.resize(static_cast<size_t>(nq));
        check(vg_search_flat_threshold(h_, queries, nq, thresholds, max_results, mask, mask_stride, r.ids.data(), r.scores.data(),
                                       r.counts.data(), nullptr));
        return r;
    }
    // Engine.SearchThreshold over a flat segment with codes and / or IVF partitions (engine/engine.go:1485-1531 over
    // flat/segment.go:447-780): the best max_results rows of the probed partitions by the score of `scan` (VG_SCAN_*), their
    // exact scores when `rerank`, then the rows within thresholds[q]; rerank false compares the scan score
    ThresholdResult SearchProbedThreshold(const float *queries, int64_t nq, const float *thresholds, int max_results, int nprobes,
                                          int scan, bool rerank, const uint8_t *mask = nullptr, int64_t mask_stride = 0)
    {
        ThresholdResult r;
        r.ids.resize(static_cast<size_t>(nq) * max_results);
        r.scores.resize(static_cast<size_t>(nq) * max_results);
        r.counts.resize(static_cast<size_t>(nq));
        check(vg_search_flat_probed_threshold(h_, queries, nq, thresholds, max_results, nprobes, scan, rerank ? 1 : 0, mask, mask_stride,
                                              r.ids.data(), r.scores.data(), r.counts.data(), nullptr));
        return r;
    }
    // the candidates SearchFlat's nomination appended to its queries' lists since the rows were attached (vg_index_flat_appended)
    int64_t FlatAppended()
    {
        int64_t n = 0;
        check(vg_index_flat_appended(h_, &n, nullptr));
        return n;
    }
    // opt-in: nominate with a bfloat16 MFMA GEMM over a bf16 copy of the rows; results stay bit-identical (vecgo_hip.h)
    void EnableBF16Filter(bool on = true) { check(vg_index_enable_bf16_filter(h_, on ? 1 : 0, nullptr)); }
    // flat.Segment.Search PQ branch (flat/segment.go:476-483,678-689)
    Result SearchPQ(const float *queries, int64_t nq, int k) { return run(nq, k, [&](Result &r) { return vg_search_pq_adc(h_, queries, nq, k, r.ids.data(), r.scores.data(), nullptr); }); }
    // opt-in: batches of SearchPQ nominated by a bfloat16 MFMA GEMM over the decoded rows, re-scored from the codes; results unchanged
    void EnablePQNomination(bool on = true) { check(vg_index_enable_pq_nomination(h_, on ? 1 : 0, nullptr)); }
    // the same without the image of the decoded rows: the GEMM's row tiles gathered from the decoded codebook by the codes
    // (8 dimensions per sub-quantizer, batches above 128 queries); the two modes are exclusive
    void EnablePQNominationFromCodes(bool on = true) { check(vg_index_enable_pq_nomination_from_codes(h_, on ? 1 : 0, nullptr)); }
    // mode: 0 off, 1 the image, 2 from the codes; held_bytes: the device memory the mode keeps resident
    struct PQNomination {
        int32_t mode;
        int64_t held_bytes;
    };
    PQNomination PQNominationInfo() const
    {
        PQNomination r{0, 0};
        check(vg_index_pq_nomination_info(h_, &r.mode, &r.held_bytes));
        return r;
    }
    // the SQ8 batch nomination without the image of the dequantised rows: the GEMM's row tiles converted from the code tiles
    // (batches above 128 queries, unfiltered, the whole segment); exclusive with EnableSQ8Nomination; results unchanged
    void EnableSQ8NominationFromCodes(bool on = true) { check(vg_index_enable_sq8_nomination_from_codes(h_, on ? 1 : 0, nullptr)); }
    // mode: 0 off, 1 the image, 2 from the codes; held_bytes: the device memory the mode keeps resident; rescanned: queries whose
    // proof failed and the scan answered, since the mode was enabled
    struct SQ8Nomination {
        int32_t mode;
        int64_t held_bytes, rescanned;
    };
    SQ8Nomination SQ8NominationInfo() const
    {
        SQ8Nomination r{0, 0, 0};
        check(vg_index_sq8_nomination_info(h_, &r.mode, &r.held_bytes, &r.rescanned));
        return r;
    }
    // SearchRaBitQ batches above 128 queries through an int8 matrix-core nomination over the sign bits (exact Hamming distances, a
    // conservative screen, exact re-score and proof; nothing resident); other batches keep the scan; results unchanged
    void EnableRaBitQNomination(bool on = true) { check(vg_index_enable_rabitq_nomination(h_, on ? 1 : 0, nullptr)); }
    // on: whether the mode is enabled; held_bytes: the device memory it keeps resident (0); rescanned: queries whose list was
    // incomplete and the scan answered, since the mode was enabled; mismatched: the VG_RABITQ_NOM_CHECK hook's count
    struct RaBitQNomination {
        int32_t on;
        int64_t held_bytes, rescanned, mismatched;
    };
    RaBitQNomination RaBitQNominationInfo() const
    {
        RaBitQNomination r{0, 0, 0, 0};
        check(vg_index_rabitq_nomination_info(h_, &r.on, &r.held_bytes, &r.rescanned, &r.mismatched));
        return r;
    }
    Result SearchRaBitQ(const float *queries, int64_t nq, int k) { return run(nq, k, [&](Result &r) { return vg_search_rabitq(h_, queries, nq, k, r.ids.data(), r.scores.data(), nullptr); }); }
    // exhaustive scan of the INT4 codes (Int4Quantizer.L2Distance per row, the DiskANN walk's own score; ascending under every
    // metric; k <= 512); mask: bit i of byte i/8 = the row takes part, one per query mask_stride apart or (0) one for the batch
    Result SearchInt4(const float *queries, int64_t nq, int k, const uint8_t *mask = nullptr, int64_t mask_stride = 0) { return run(nq, k, [&](Result &r) { return vg_search_int4(h_, queries, nq, k, mask, mask_stride, r.ids.data(), r.scores.data(), nullptr); }); }
    // IVF partitions (flat/segment.go:187-207) and the probed scan of flat.Segment.Search (:727-749):
    // scan = VG_SCAN_F32 / VG_SCAN_PQ / VG_SCAN_SQ8, nprobes <= 0 means 1 as in the reference
    void SetPartitions(const float *centroids, const uint32_t *part_offsets, int num_partitions)
    {
        check(vg_index_set_partitions(h_, centroids, part_offsets, num_partitions, nullptr));
    }
    // Segment.Search with a row filter (flat/segment.go:631-635): mask bit i of byte i/8 = filter.Matches(i)
    Result SearchFiltered(const float *queries, int64_t nq, int k, int nprobes, int scan, const uint8_t *mask, int64_t mask_stride) { return run(nq, k, [&](Result &r) { return vg_search_flat_filtered(h_, queries, nq, k, nprobes, scan, mask, mask_stride, r.ids.data(), r.scores.data(), nullptr); }); }
    // the engine's bitmap strategy (engine/search.go:602-736): only the rows the mask keeps are fetched and scored; the host picks it
    // for selective filters from the masks' counts; partitions are ignored; k <= 16384
    Result SearchPrefilter(const float *queries, int64_t nq, int k, const uint8_t *mask, int64_t mask_stride) { return run(nq, k, [&](Result &r) { return vg_search_flat_prefilter(h_, queries, nq, k, mask, mask_stride, r.ids.data(), r.scores.data(), nullptr); }); }
    Result SearchProbed(const float *queries, int64_t nq, int k, int nprobes, int scan) { return run(nq, k, [&](Result &r) { return vg_search_flat_probed(h_, queries, nq, k, nprobes, scan, r.ids.data(), r.scores.data(), nullptr); }); }
    // hnsw.Insert over the segment's rows (hnsw.go:713-984, ids and levels of ApplyInsert); replaces the segment's graph
    void BuildHNSW(int m = 32, int efConstruction = 300, int maxBatch = 8192, int growthDiv = 32)
    {
        check(vg_hnsw_build(h_, m, efConstruction, maxBatch, growthDiv, nullptr));
    }
    // hnsw.ApplyInsert for `count` rows appended as rows n .. n+count-1 (vg_hnsw_insert); rows host or device
    void InsertHNSW(const float *rows, int64_t count, int m = 32, int ef = 300, int maxBatch = 8192, int growthDiv = 32)
    {
        check(vg_hnsw_insert(h_, rows, count, m, ef, maxBatch, growthDiv, nullptr));
    }
    // hnsw.Compact (compact.go:16-34) under the segment's tombstones (vg_hnsw_compact): repair, prune, clear
    vg_hnsw_compact_stats CompactHNSW(int ef = 300, int maxBatch = 8192)
    {
        vg_hnsw_compact_stats stats{};
        check(vg_hnsw_compact(h_, ef, maxBatch, &stats, nullptr));
        return stats;
    }
    // diskann.Writer.buildGraph over the segment's rows (writer.go:362-460); replaces the segment's Vamana graph
    void BuildVamana(int r = 64, int l = 100, float alpha = 1.2f, const uint32_t *initGraph = nullptr, uint64_t seed = 0,
                     int maxBatch = 8192, int growthDiv = 32)
    {
        check(vg_vamana_build(h_, r, l, alpha, initGraph, seed, maxBatch, growthDiv, nullptr));
    }
    // FreshVamana.Insert (fresh_vamana.go:178-222) for `count` rows appended as rows n .. n+count-1 (vg_vamana_insert); rows and
    // deleted (bit i of byte i/8 = node i is deleted, the rows before the call; null = none) host or device
    void InsertVamana(const float *rows, int64_t count, int r = 64, int l = 100, float alpha = 1.2f, const uint8_t *deleted = nullptr,
                      uint64_t seed = 0, int maxBatch = 8192, int growthDiv = 32)
    {
        check(vg_vamana_insert(h_, rows, count, r, l, alpha, deleted, seed, maxBatch, growthDiv, nullptr));
    }
    // FreshVamana.consolidate (fresh_vamana.go:803-867) under the caller's deleted bits (vg_vamana_consolidate; bit i of byte
    // i/8, host or device, null = none): every live node that lists a deleted one is searched for and pruned again
    vg_vamana_consolidate_stats ConsolidateVamana(const uint8_t *deleted, int l = 100, float alpha = 1.2f, int maxBatch = 8192)
    {
        vg_vamana_consolidate_stats stats{};
        check(vg_vamana_consolidate(h_, l, alpha, deleted, maxBatch, &stats, nullptr));
        return stats;
    }
    // diskann.Writer.reorderBFS (reorder.go:14-157): the graph and every per-row array into BFS order; perm[new] = old,
    // invPerm[old] = new (either may be null; host or device)
    void ReorderVamanaBFS(uint32_t *perm, uint32_t *invPerm) { check(vg_vamana_reorder_bfs(h_, perm, invPerm, nullptr)); }
    // flat.Writer.Flush's partitioning and quantization (flat/writer.go:99-223) where the rows lie: k-means + the stable
    // regrouping by partition (perm[new] = old, invPerm[old] = new; either may be null), then the quantizer (VG_QUANT_NONE /
    // _SQ8 with sq / _PQ with pq = ProductQuantizer(dim, pqM ? pqM : dim / 8, 256)) trained on and applied to the new order
    void FlatBuild(int numPartitions, int quantization, std::shared_ptr<quantization::ScalarQuantizer> sq,
                   std::shared_ptr<quantization::ProductQuantizer> pq, uint32_t *perm, uint32_t *invPerm, uint64_t seed = 0,
                   int pqM = 0, int kmeansIters = 0, int pqIters = 0)
    {
        check(vg_flat_build(h_, numPartitions, quantization, pqM, kmeansIters, pqIters, seed, sq ? sq->handle() : nullptr,
                            pq ? pq->handle() : nullptr, perm, invPerm, nullptr));
        if (quantization == VG_QUANT_SQ8) sq_ = std::move(sq);
        if (quantization == VG_QUANT_PQ) pq_ = std::move(pq);
    }
    // the file Writer.Flush writes (flat/writer.go:312-470) for this segment; ids in the segment's row order (null: 0 .. rows-1),
    // metadata / blockStats: the host's serialised sections (empty: the writer's bytes for rows without documents)
    std::vector<uint8_t> WriteFlat(uint64_t segmentID, const uint64_t *ids = nullptr, const std::vector<uint8_t> *metadata = nullptr,
                                   const std::vector<uint8_t> *blockStats = nullptr)
    {
        const int64_t size = vg_segment_flat_image_size(h_, metadata ? static_cast<int64_t>(metadata->size()) : -1,
                                                        blockStats ? static_cast<int64_t>(blockStats->size()) : -1);
        if (size < 0) check(VG_ERR_UNSUPPORTED);
        std::vector<uint8_t> image(static_cast<size_t>(size));
        static const uint8_t none = 0;  // (an empty section still travels as a non-null pointer)
        int64_t written = 0;
        check(vg_segment_write_flat(h_, segmentID, ids, metadata ? (metadata->empty() ? &none : metadata->data()) : nullptr,
                                    metadata ? static_cast<int64_t>(metadata->size()) : 0,
                                    blockStats ? (blockStats->empty() ? &none : blockStats->data()) : nullptr,
                                    blockStats ? static_cast<int64_t>(blockStats->size()) : 0, image.data(), size, &written, nullptr));
        return image;
    }
    // diskann.Writer.Write up to Flush (diskann/writer.go:217-253) where the rows lie: the quantizer (VG_QUANT_NONE / _PQ with
    // pq = ProductQuantizer(dim, pqM, 256) / _RABITQ / _INT4 with iq) trained on and applied to the rows in add order, then
    // BuildVamana, then ReorderVamanaBFS (perm[new] = old, invPerm[old] = new; either may be null).  Returns the VG_QUANT_* kind
    // of the codes now on the segment: VG_QUANT_NONE for PQ over fewer than 256 rows (trainPQ, :276-279)
    int DiskANNBuild(int r, int l, float alpha, int quantization, std::shared_ptr<quantization::ProductQuantizer> pq,
                     std::shared_ptr<quantization::Int4Quantizer> iq, uint32_t *perm, uint32_t *invPerm, uint64_t seed = 0,
                     int pqM = 0, int pqIters = 0, int maxBatch = 8192, int growthDiv = 32)
    {
        int32_t used = VG_QUANT_NONE;
        check(vg_diskann_build(h_, r, l, alpha, quantization, pqM, pqIters, seed, maxBatch, growthDiv, pq ? pq->handle() : nullptr,
                               iq ? iq->handle() : nullptr, perm, invPerm, &used, nullptr));
        if (used == VG_QUANT_PQ) pq_ = std::move(pq);
        if (used == VG_QUANT_INT4) iq_ = std::move(iq);
        return used;
    }
    // the file Writer.Flush writes (diskann/writer.go:645-856) for this segment; searchListSize: the header's L (0 = 100);
    // compressionType: recorded, the sections are raw; ids in the segment's row order (null: 0 .. rows-1); metadata /
    // metadataIndex: the host's serialised sections (null: the writer's bytes for rows without documents)
    std::vector<uint8_t> WriteDiskANN(uint64_t segmentID, int searchListSize = 0, int compressionType = 1, const uint64_t *ids = nullptr,
                                      const std::vector<uint8_t> *metadata = nullptr, const std::vector<uint8_t> *metadataIndex = nullptr)
    {
        const int64_t size = vg_segment_diskann_image_size(h_, metadata ? static_cast<int64_t>(metadata->size()) : -1,
                                                           metadataIndex ? static_cast<int64_t>(metadataIndex->size()) : -1);
        std::vector<uint8_t> image(static_cast<size_t>(size < 0 ? 1 : size));  // (size < 0: the call below names the refusal)
        static const uint8_t none = 0;  // (an empty section still travels as a non-null pointer)
        int64_t written = 0;
        check(vg_segment_write_diskann(h_, segmentID, searchListSize, compressionType, ids,
                                       metadata ? (metadata->empty() ? &none : metadata->data()) : nullptr,
                                       metadata ? static_cast<int64_t>(metadata->size()) : 0,
                                       metadataIndex ? (metadataIndex->empty() ? &none : metadataIndex->data()) : nullptr,
                                       metadataIndex ? static_cast<int64_t>(metadataIndex->size()) : 0, image.data(), size < 0 ? 0 : size,
                                       &written, nullptr));
        return image;
    }
    // the Vamana graph (n * r ids, VG_INVALID_ID = empty slot) and its entry point
    std::vector<uint32_t> VamanaGraph(int *r, uint32_t *entry) const
    {
        check(vg_index_get_vamana_graph(h_, r, entry, nullptr, nullptr));
        std::vector<uint32_t> g(static_cast<size_t>(n_) * *r);
        check(vg_index_get_vamana_graph(h_, nullptr, nullptr, g.data(), nullptr));
        return g;
    }
    // the graph walk scored from PQ codes (candidates for Rerank, engine/search.go:914-965)
    Result SearchHNSWPQ(const float *queries, int64_t nq, int k, int ef) { return run(nq, k, [&](Result &r) { return vg_search_hnsw_pq(h_, queries, nq, k, ef, r.ids.data(), r.scores.data(), nullptr, nullptr); }); }
    // hnsw.KNNSearch (hnsw.go:1650-1755)
    Result SearchHNSW(const float *queries, int64_t nq, int k, int ef) { return run(nq, k, [&](Result &r) { return vg_search_hnsw(h_, queries, nq, k, ef, r.ids.data(), r.scores.data(), nullptr, nullptr); }); }
    // hnsw.BruteSearch + scanSegment (hnsw.go:2021-2101; VG_BRUTE_SCAN) / searchBitmap (:2240-2263; VG_BRUTE_BITMAP)
    Result SearchHNSWBrute(const float *queries, int64_t nq, int k, int mode, const uint8_t *mask = nullptr, int64_t mask_stride = 0) { return run(nq, k, [&](Result &r) { return vg_search_hnsw_brute(h_, queries, nq, k, mode, mask, mask_stride, r.ids.data(), r.scores.data(), nullptr); }); }
    // diskann searchInternal (diskann/segment.go:503-706); kind 0 fp32, 1 PQ, 2 RaBitQ
    // searchInternal with a row filter (diskann/segment.go:616-627): mask bit i of byte i/8 = filter.Matches(i)
    Result SearchVamanaFiltered(const float *queries, int64_t nq, int k, int kind, const uint8_t *mask, int64_t mask_stride) { return run(nq, k, [&](Result &r) { return vg_search_vamana_filtered(h_, queries, nq, k, kind, mask, mask_stride, r.ids.data(), r.scores.data(), nullptr, nullptr); }); }
    Result SearchVamana(const float *queries, int64_t nq, int k, int kind) { return run(nq, k, [&](Result &r) { return vg_search_vamana(h_, queries, nq, k, kind, r.ids.data(), r.scores.data(), nullptr, nullptr); }); }
    // FreshVamana.Search / SearchWithFilter (fresh_vamana.go:272-364): l = the index's search list size, deleted as for
    // InsertVamana, mask = nullptr: Search.  counts[q] rows found, the rest padded
    ThresholdResult SearchVamanaFresh(const float *queries, int64_t nq, int k, int l = 100, const uint8_t *deleted = nullptr,
                                      const uint8_t *mask = nullptr, int64_t mask_stride = 0)
    {
        ThresholdResult r;
        r.ids.resize(static_cast<size_t>(nq) * k);
        r.scores.resize(static_cast<size_t>(nq) * k);
        r.counts.resize(static_cast<size_t>(nq));
        check(vg_search_vamana_fresh(h_, queries, nq, k, l, deleted, mask, mask_stride, r.ids.data(), r.scores.data(), r.counts.data(),
                                     nullptr));
        return r;
    }
    // Engine.SearchThreshold's DiskANN leg (engine/engine.go:1485-1531): SearchVamanaFiltered(q, max_results), then the rows within
    // thresholds[q] (<= for L2, >= for Dot / Cosine) in walk order; mask = nullptr: no filter.  max_results <= 16384
    ThresholdResult SearchVamanaThreshold(const float *queries, int64_t nq, const float *thresholds, int max_results, int kind,
                                          const uint8_t *mask = nullptr, int64_t mask_stride = 0)
    {
        ThresholdResult r;
        r.ids.resize(static_cast<size_t>(nq) * max_results);
        r.scores.resize(static_cast<size_t>(nq) * max_results);
        r.counts.resize(static_cast<size_t>(nq));
        check(vg_search_vamana_threshold(h_, queries, nq, thresholds, max_results, kind, mask, mask_stride, r.ids.data(),
                                         r.scores.data(), r.counts.data(), nullptr, nullptr));
        return r;
    }
    // Segment.Rerank (flat/segment.go:754-780) + top-k
    Result Rerank(const float *queries, int64_t nq, const uint32_t *cand, int nc, int k) { return run(nq, k, [&](Result &r) { return vg_rerank(h_, queries, nq, cand, nc, k, r.ids.data(), r.scores.data(), nullptr); }); }

    int64_t Rows() const { return n_; }

    // Where Engine.CompactWithContext's rows went (engine/compaction.go:159-213): oldToNew over the concatenated source rows
    // (VG_INVALID_ID = deleted), newSource / newRow per row of the new segment
    struct Moves {
        std::vector<uint32_t> oldToNew;
        std::vector<int32_t> newSource;
        std::vector<uint32_t> newRow;
    };
    // The compaction's Iterate loop over resident segments (compaction.go:173-218; vg_index_merge): the rows of sources[0],
    // then sources[1], ... whose bit in deleted[s] (bit i of byte i/8, host or device; a null entry or an empty vector = none
    // deleted) is clear, as a new segment with fp32 rows only
    static std::unique_ptr<Segment> Merge(std::shared_ptr<Context> ctx, const std::vector<const Segment *> &sources,
                                          const std::vector<const uint8_t *> &deleted, Moves *moves = nullptr)
    {
        if (sources.empty() || (!deleted.empty() && deleted.size() != sources.size()))
            throw std::invalid_argument("Segment::Merge: at least one source, and no bitmaps or one (may be null) per source");
        std::vector<const vg_index *> hs;
        int64_t total = 0;
        for (const Segment *s : sources) {
            if (!s) throw std::invalid_argument("Segment::Merge: null source");
            hs.push_back(s->h_);
            total += s->n_;
        }
        Moves m;
        m.oldToNew.resize(static_cast<size_t>(total));
        m.newSource.resize(static_cast<size_t>(total));
        m.newRow.resize(static_cast<size_t>(total));
        vg_index *out = nullptr;
        check(vg_index_merge(ctx->handle(), hs.data(), deleted.empty() ? nullptr : deleted.data(), static_cast<int32_t>(hs.size()), &out,
                             m.oldToNew.data(), m.newSource.data(), m.newRow.data(), nullptr));
        int64_t live = 0;
        for (uint32_t v : m.oldToNew) live += v != VG_INVALID_ID;
        m.newSource.resize(static_cast<size_t>(live));
        m.newRow.resize(static_cast<size_t>(live));
        if (moves) *moves = std::move(m);
        return std::unique_ptr<Segment>(new Segment(std::move(ctx), out, live, sources[0]->dim_));
    }
    // Engine.CompactWithContext's choice of writer (compaction.go:86-152) for totalRows source rows, deleted ones included:
    // true = DiskANN (from diskannThreshold rows up, 0 = 10000), else flat with *k = max(1, totalRows / 8192) partitions
    static bool CompactionPlan(int64_t totalRows, int64_t diskannThreshold, int *k)
    {
        if (totalRows >= (diskannThreshold > 0 ? diskannThreshold : 10000)) return true;
        *k = totalRows / 8192 < 1 ? 1 : static_cast<int>(totalRows / 8192);
        return false;
    }
    // Merge, then the writer CompactionPlan chooses: FlatBuild(k, flatQuantization, sq, pq) or DiskANNBuild(r, l, alpha,
    // diskannQuantization, pq, iq).  *diskann says which; moves holds the FINAL positions, Merge's maps composed with the
    // builder's perm / invPerm (the reference's flat NewRowID is right only for k = 1, compaction.go:205-206)
    static std::unique_ptr<Segment> Compact(std::shared_ptr<Context> ctx, const std::vector<const Segment *> &sources,
                                            const std::vector<const uint8_t *> &deleted, Moves *moves, bool *diskann,
                                            int64_t diskannThreshold = 0, int flatQuantization = VG_QUANT_NONE,
                                            std::shared_ptr<quantization::ScalarQuantizer> sq = nullptr,
                                            std::shared_ptr<quantization::ProductQuantizer> pq = nullptr, int r = 64, int l = 100,
                                            float alpha = 1.2f, int diskannQuantization = VG_QUANT_NONE,
                                            std::shared_ptr<quantization::Int4Quantizer> iq = nullptr, uint64_t seed = 0, int pqM = 0)
    {
        int64_t total = 0;
        for (const Segment *s : sources) {
            if (!s) throw std::invalid_argument("Segment::Compact: null source");
            total += s->n_;
        }
        int k = 0;
        const bool ann = CompactionPlan(total, diskannThreshold, &k);
        Moves m;
        std::unique_ptr<Segment> merged = Merge(std::move(ctx), sources, deleted, &m);
        std::vector<uint32_t> perm(static_cast<size_t>(merged->n_)), inv(static_cast<size_t>(merged->n_));
        if (ann)
            merged->DiskANNBuild(r, l, alpha, diskannQuantization, std::move(pq), std::move(iq), perm.data(), inv.data(), seed, pqM);
        else
            merged->FlatBuild(k, flatQuantization, std::move(sq), std::move(pq), perm.data(), inv.data(), seed, pqM);
        Moves f;
        f.oldToNew = m.oldToNew;
        for (uint32_t &v : f.oldToNew)
            if (v != VG_INVALID_ID) v = inv[v];
        for (uint32_t p : perm) {
            f.newSource.push_back(m.newSource[p]);
            f.newRow.push_back(m.newRow[p]);
        }
        if (moves) *moves = std::move(f);
        if (diskann) *diskann = ann;
        return merged;
    }

private:
    // a handle the library created (vg_index_merge)
    Segment(std::shared_ptr<Context> ctx, vg_index *h, int64_t rows, int dim) : ctx_(std::move(ctx)), h_(h), n_(rows), dim_(dim) {}
    template <typename F>
    Result run(int64_t nq, int k, F f)
    {
        Result r;
        r.ids.resize(static_cast<size_t>(nq) * k);
        r.scores.resize(static_cast<size_t>(nq) * k);
        check(f(r));
        return r;
    }
    std::shared_ptr<Context> ctx_;
    std::shared_ptr<quantization::ProductQuantizer> pq_;
    std::shared_ptr<quantization::ScalarQuantizer> sq_;
    std::shared_ptr<quantization::Int4Quantizer> iq_;
    vg_index *h_ = nullptr;
    int64_t n_;
    int dim_;
};

// ---- metadata filters on the device -------------------------------------------------------------------------------------
namespace metadata {

// metadata.Operator as vg_filter_clause.op
enum class Op : int32_t { Eq = VG_FILTER_EQ, Ne = VG_FILTER_NE, Lt = VG_FILTER_LT, Lte = VG_FILTER_LTE, Gt = VG_FILTER_GT, Gte = VG_FILTER_GTE, In = VG_FILTER_IN };
enum class MaskOp : int32_t { And = VG_MASK_AND, AndNot = VG_MASK_ANDNOT, Or = VG_MASK_OR, Xor = VG_MASK_XOR };

// One metadata.Filter against a resident column: `value` is read for a float64 column, `code` (Eq) and `codes` (In) for a
// dictionary-coded one; VG_INVALID_ID is the code of a value the dictionary does not hold (no row matches it).
struct Filter {
    int32_t field = 0;
    Op op = Op::Eq;
    double value = 0.0;
    uint32_t code = VG_INVALID_ID;
    std::vector<uint32_t> codes;
};
using FilterSet = std::vector<Filter>;  // metadata.FilterSet: the AND of its filters; empty = every row

// The resident metadata columns of one segment (vg_columns).  The value -> code dictionary, Set / Delete bookkeeping and
// uploading a column again after writes stay the host's.
class Columns {
public:
    Columns(std::shared_ptr<Context> ctx, int64_t rows) : ctx_(std::move(ctx)), rows_(rows) { check(vg_columns_create(ctx_->handle(), rows, &h_)); }
    ~Columns() { vg_columns_destroy(h_); }
    Columns(const Columns &) = delete;
    Columns &operator=(const Columns &) = delete;
    // values[rows]; present: bit i of byte i/8 = row i has a value, nullptr = every row (ints as float64(I64))
    void SetFloat64(int32_t field, const double *values, const uint8_t *present = nullptr) { check(vg_columns_set_f64(h_, field, values, present, nullptr)); }
    // codes[rows], VG_INVALID_ID = the row has no value
    void SetCodes(int32_t field, const uint32_t *codes) { check(vg_columns_set_codes(h_, field, codes, nullptr)); }
    void Drop(int32_t field) { check(vg_columns_drop(h_, field)); }
    int64_t rows() const { return rows_; }
    vg_columns *handle() const { return h_; }
    const std::shared_ptr<Context> &context() const { return ctx_; }

private:
    std::shared_ptr<Context> ctx_;
    vg_columns *h_ = nullptr;
    int64_t rows_;
};

// The row masks of a query batch in device memory (vg_mask_alloc): data() / stride() go to the searches' mask /
// mask_stride as they are; counts[q] = the rows query q's filter set matches.
class DeviceMasks {
public:
    DeviceMasks(std::shared_ptr<Context> ctx, int64_t nq, int64_t rows) : ctx_(std::move(ctx)), nq_(nq), rows_(rows), stride_(((rows + 7) / 8 + 7) & ~int64_t(7))
    {
        check(vg_mask_alloc(ctx_->handle(), nq_ * stride_, &p_));
        counts.assign(static_cast<size_t>(nq), 0);
    }
    ~DeviceMasks() { vg_mask_free(ctx_->handle(), p_); }
    DeviceMasks(const DeviceMasks &) = delete;
    DeviceMasks &operator=(const DeviceMasks &) = delete;
    uint8_t *data() const { return p_; }
    int64_t stride() const { return stride_; }
    int64_t size() const { return nq_; }
    // mask[q] = mask[q] op hostMask for every q: joins a mask made on the host (`contains`, string ranges)
    void Combine(MaskOp op, const uint8_t *hostMask)
    {
        check(vg_mask_combine(ctx_->handle(), static_cast<int32_t>(op), p_, stride_, hostMask, 0, nq_, rows_, nullptr));
    }
    // counts the masks again (after Combine)
    const std::vector<int64_t> &Popcount()
    {
        if (nq_ > 0) check(vg_mask_popcount(ctx_->handle(), p_, stride_, nq_, rows_, counts.data(), nullptr));
        return counts;
    }
    // FilterResult.ToArrayInto for the batch (vg_mask_to_rows): [size() * outStride] row ids, ascending per query, at most
    // outStride each, the rest VG_INVALID_ID; counts is refreshed (all set bits, also past outStride)
    std::vector<uint32_t> Rows(int64_t outStride)
    {
        std::vector<uint32_t> rows(static_cast<size_t>(nq_ * outStride));
        if (nq_ > 0) check(vg_mask_to_rows(ctx_->handle(), p_, stride_, nq_, rows_, rows.empty() ? nullptr : rows.data(), outStride, counts.data(), nullptr));
        return rows;
    }
    std::vector<int64_t> counts;

private:
    std::shared_ptr<Context> ctx_;
    uint8_t *p_ = nullptr;
    int64_t nq_, rows_, stride_;
};

// UnifiedIndex.EvaluateFilter (internal/metadata/unified.go:279-416) for a batch (vg_filter_evaluate): one mask per filter
// set, the deleted rows (bit i of byte i/8, nullptr = none) cleared from every one.  Only the predicates cross to the device.
inline std::unique_ptr<DeviceMasks> EvaluateFilters(const Columns &cols, const std::vector<FilterSet> &sets, const uint8_t *deleted = nullptr)
{
    std::vector<vg_filter_clause> clauses;
    std::vector<int32_t> off{0};
    std::vector<uint32_t> codes;
    for (const FilterSet &fs : sets) {
        for (const Filter &f : fs) {
            vg_filter_clause c{};
            c.field = f.field;
            c.op = static_cast<int32_t>(f.op);
            c.value = f.value;
            c.code = f.code;
            if (f.op == Op::In) {
                c.set_begin = static_cast<int32_t>(codes.size());
                c.set_count = static_cast<int32_t>(f.codes.size());
                codes.insert(codes.end(), f.codes.begin(), f.codes.end());
            }
            clauses.push_back(c);
        }
        off.push_back(static_cast<int32_t>(clauses.size()));
    }
    const int64_t nq = static_cast<int64_t>(sets.size());
    auto masks = std::make_unique<DeviceMasks>(cols.context(), nq, cols.rows());
    check(vg_filter_evaluate(cols.handle(), clauses.empty() ? nullptr : clauses.data(), off.data(), nq, codes.empty() ? nullptr : codes.data(),
                             static_cast<int64_t>(codes.size()), deleted, masks->data(), masks->stride(), masks->counts.data(), nullptr));
    return masks;
}

}  // namespace metadata

// ---- hybrid search: the resident BM25 index and Reciprocal Rank Fusion ---------------------------------------------------
namespace lexical {

// What a batch of lexical or fused searches answers: [nq * k] ids / scores best first (VG_INVALID_ID / -Inf behind a short
// list) and the hits per query.
struct Hits {
    std::vector<uint32_t> ids;
    std::vector<float> scores;
    std::vector<int32_t> counts;
};

// lexical/bm25.MemoryIndex resident on the device (vg_bm25): CSR postings in strictly ascending doc order (host arrays are
// checked), doc lengths, idx.totalLength / idx.docCount and the doc -> id map (nullptr: the doc id itself).  The tokeniser, the
// term dictionary and the idf stay the host's; writes reach the index through Update (vg_bm25_update), which rewrites the image
// on the device: term ids are stable, a failed call leaves the index as it was.
class Bm25 {
public:
    Bm25(std::shared_ptr<Context> ctx, int64_t nDocs, const std::vector<int64_t> &termOff, const std::vector<uint32_t> &postDoc,
         const std::vector<uint32_t> &postTf, const std::vector<uint32_t> &docLen, int64_t totalLength, int64_t docCount,
         const uint32_t *docToId = nullptr)
        : ctx_(std::move(ctx))
    {
        check(vg_bm25_create(ctx_->handle(), nDocs, static_cast<int64_t>(termOff.size()) - 1, termOff.data(), postDoc.data(), postTf.data(), docLen.data(),
                             totalLength, docCount, docToId, &h_));
    }
    ~Bm25() { vg_bm25_destroy(h_); }
    // an index without docs or terms that Update fills (vg_bm25_create_empty); withDocToId: results go through the ids Update is given
    static std::unique_ptr<Bm25> Empty(std::shared_ptr<Context> ctx, bool withDocToId = false)
    {
        std::unique_ptr<Bm25> b(new Bm25());
        b->ctx_ = std::move(ctx);
        check(vg_bm25_create_empty(b->ctx_->handle(), withDocToId ? 1 : 0, &b->h_));
        return b;
    }
    // a batch of MemoryIndex.Delete followed by a batch of Add (vg_bm25_update): the docs delDocs go, then added doc i = addDocs[i] of
    // length addLen[i] arrives with the postings (addTerms[p], addTf[p]), p in addOff[i] .. addOff[i + 1]; addIds: the ids the docs
    // are reported under (an index with a doc -> id map), empty otherwise.  nDocs / nTerms: the sizes afterwards (never smaller).
    void Update(const std::vector<uint32_t> &delDocs, const std::vector<uint32_t> &addDocs, const std::vector<uint32_t> &addLen,
                const std::vector<uint32_t> &addIds, const std::vector<int64_t> &addOff, const std::vector<uint32_t> &addTerms,
                const std::vector<uint32_t> &addTf, int64_t nDocs, int64_t nTerms, int64_t totalLength, int64_t docCount)
    {
        check(vg_bm25_update(h_, delDocs.data(), static_cast<int64_t>(delDocs.size()), addDocs.data(), addLen.data(),
                             addIds.empty() ? nullptr : addIds.data(), static_cast<int64_t>(addDocs.size()), addOff.data(), addTerms.data(),
                             addTf.data(), nDocs, nTerms, totalLength, docCount, nullptr));
    }
    // the resident image copied out (vg_bm25_export): what persists an index the host never built
    struct Image {
        std::vector<int64_t> termOff;
        std::vector<uint32_t> postDoc, postTf, docLen, docToId;
    };
    Image Export(bool withDocToId)
    {
        int64_t docs = 0, terms = 0, postings = 0;
        check(vg_bm25_stats(h_, &docs, &terms, &postings, nullptr));
        Image im;
        im.termOff.resize(static_cast<size_t>(terms) + 1);
        im.postDoc.resize(static_cast<size_t>(postings));
        im.postTf.resize(static_cast<size_t>(postings));
        im.docLen.resize(static_cast<size_t>(docs));
        if (withDocToId) im.docToId.resize(static_cast<size_t>(docs));
        check(vg_bm25_export(h_, im.termOff.data(), im.postDoc.data(), im.postTf.data(), im.docLen.data(), withDocToId ? im.docToId.data() : nullptr,
                             nullptr));
        return im;
    }
    Bm25(const Bm25 &) = delete;
    Bm25 &operator=(const Bm25 &) = delete;
    // MemoryIndex.Search for a batch: query q's term ids termIds[termOff[q] .. termOff[q + 1]) with the caller's idf
    // (math.Log(1 + (N - n + 0.5) / (n + 0.5))) per entry
    Hits Search(const std::vector<int32_t> &termOff, const std::vector<uint32_t> &termIds, const std::vector<double> &idf, int k)
    {
        const int64_t nq = static_cast<int64_t>(termOff.size()) - 1;
        Hits r;
        r.ids.resize(static_cast<size_t>(nq) * k);
        r.scores.resize(static_cast<size_t>(nq) * k);
        r.counts.assign(static_cast<size_t>(nq), 0);
        check(vg_bm25_search(h_, termOff.data(), termIds.data(), idf.data(), nq, k, r.ids.data(), r.scores.data(), r.counts.data(), nullptr));
        return r;
    }
    // the queries whose tied scores went through the reference's heap on the device
    int64_t Replayed()
    {
        int64_t n = 0;
        check(vg_bm25_replayed(h_, &n, nullptr));
        return n;
    }
    int64_t ResidentBytes()
    {
        int64_t bytes = 0;
        check(vg_bm25_stats(h_, nullptr, nullptr, nullptr, &bytes));
        return bytes;
    }
    vg_bm25 *handle() const { return h_; }

private:
    Bm25() = default;
    std::shared_ptr<Context> ctx_;
    vg_bm25 *h_ = nullptr;
};

// The fusion of Engine.HybridSearch (engine.go:1560-1602) for a batch (vg_rrf_fuse): list A sets 1 / float32(rrfK + rank + 1)
// per id, list B adds it; the best k by score, ties by ascending id.
inline Hits FuseRRF(Context &ctx, int64_t nq, const uint32_t *aIds, const int32_t *aCounts, int64_t aStride, const uint32_t *bIds,
                    const int32_t *bCounts, int64_t bStride, int rrfK, int k)
{
    Hits r;
    r.ids.resize(static_cast<size_t>(nq) * k);
    r.scores.resize(static_cast<size_t>(nq) * k);
    r.counts.assign(static_cast<size_t>(nq), 0);
    check(vg_rrf_fuse(ctx.handle(), nq, aIds, aCounts, aStride, bIds, bCounts, bStride, rrfK, k, r.ids.data(), r.scores.data(), r.counts.data(), nullptr));
    return r;
}

}  // namespace lexical

}  // namespace vecgo
