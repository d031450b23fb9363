// tests/adapter_shim/adapter_io.hpp — TEST INFRASTRUCTURE.  What the adapter_*_main.cpp programs share: the files of length-prefixed blocks {int64 nbytes; bytes} the
// tests write and read (tests/loop_match_cases.py write_blocks / read_blocks), the key point as those files hold it, and cv::Mat from raw arrays.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvshim.hpp"

namespace adapter_io {

// an input file's blocks: by index (in[3], in.size()) or one after the other (in.get<T>(&count))
struct Blocks {
    std::vector<std::vector<uint8_t>> b;
    size_t next = 0;
    bool load(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return false;
        int64_t n;
        while (std::fread(&n, 8, 1, f) == 1) { b.emplace_back((size_t)n); if (n && std::fread(b.back().data(), 1, (size_t)n, f) != (size_t)n) return false; }
        std::fclose(f);
        return true;
    }
    size_t size() const { return b.size(); }
    const std::vector<uint8_t>& operator[](size_t i) const { return b.at(i); }
    template <typename T> const T* get(size_t* count = nullptr) { auto& v = b.at(next++); if (count) *count = v.size() / sizeof(T); return (const T*)v.data(); }
};
template <class T> inline void write_block(FILE* f, const T* p, size_t n) { const int64_t k = (int64_t)(n * sizeof(T)); std::fwrite(&k, 8, 1, f); if (n) std::fwrite(p, sizeof(T), n, f); }

struct KP7 { float x, y, size, angle, response; int32_t octave, class_id; };
inline cv::KeyPoint to_keypoint(const KP7& k) { return cv::KeyPoint(k.x, k.y, k.size, k.angle, k.response, k.octave, k.class_id); }
inline void to_keypoints(const KP7* k, int n, std::vector<cv::KeyPoint>& out) { out.resize(n); for (int i = 0; i < n; i++) out[i] = to_keypoint(k[i]); }

inline cv::Mat mat_f32(int r, int c, const float* src) { cv::Mat m(r, c, CV_32F); std::memcpy(m.data, src, sizeof(float) * r * c); return m; }
inline cv::Mat desc_mat(int n, const uint8_t* src) { cv::Mat m(n, 32, CV_8UC1); if (n) std::memcpy(m.data, src, (size_t)n * 32); return m; }

}  // namespace adapter_io
