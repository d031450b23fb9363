// tests/adapter_shim/adapter_kfdb_main.cpp — TEST INFRASTRUCTURE.  Planar_SLAM::KeyFrameDatabase of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_KFDB) executed on
// stand-in key frames and frames that hold what the adapter reads: mBowVec, GetBestCovisibilityKeyFrames, GetConnectedKeyFrames.  Same input as the fixture generator's
// driver (tools/kfdb_golden/ref_kfdb_main.cpp; written by tests/kfdb_cases.py write_input): the add() / erase() calls, then the queries one after the other on the
// same database.
//   adapter_kfdb <in.bin> <out.bin>
// out.bin: per query n_kf x float the score members before the query, int32 n_cand, n_cand x int32 slot of the returned vector, n_kf x float the members after it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace Planar_SLAM {
typedef std::map<unsigned int, double> BowVector;      // DBoW2::BowVector is a std::map<WordId, WordValue>
class KeyFrame {
public:
    long unsigned int mnId = 0;
    BowVector mBowVec;
    std::set<KeyFrame*> connected;
    std::vector<KeyFrame*> covisible;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
    }
};
class Frame {
public:
    long unsigned int mnId = 0;
    BowVector mBowVec;
};
struct ORBVocabulary {};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_KFDB
#include "planar_adapters.hpp"

using namespace Planar_SLAM;

namespace {
FILE* fi;
template <typename T> T rd() { T v; if (std::fread(&v, sizeof(T), 1, fi) != 1) std::exit(4); return v; }
void read_bow(BowVector& v) {
    const int n = rd<int32_t>();
    std::vector<int32_t> w(n);
    for (int i = 0; i < n; i++) w[i] = rd<int32_t>();
    for (int i = 0; i < n; i++) v[(unsigned int)w[i]] = rd<double>();
}
struct Database : KeyFrameDatabase {
    using KeyFrameDatabase::KeyFrameDatabase;
    float member(KeyFrame* kf, int mode) { const auto it = slot_of_.find(kf); return it == slot_of_.end() ? 0.f : slots_[it->second].score[mode]; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    fi = std::fopen(argv[1], "rb");
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    const int n_kf = rd<int32_t>(), n_ops = rd<int32_t>(), n_q = rd<int32_t>();
    (void)rd<int32_t>();
    std::vector<KeyFrame> kfs(n_kf);
    std::vector<std::vector<int32_t>> cov(n_kf, std::vector<int32_t>(10));
    for (int j = 0; j < n_kf; j++) {
        kfs[j].mnId = j + 1;
        read_bow(kfs[j].mBowVec);
        for (int t = 0; t < 10; t++) cov[j][t] = rd<int32_t>();
    }
    for (int j = 0; j < n_kf; j++)
        for (int t = 0; t < 10; t++) if (cov[j][t] >= 0) kfs[j].covisible.push_back(&kfs[cov[j][t]]);
    ORBVocabulary voc;
    Database db(voc);
    for (int i = 0; i < n_ops; i++) {
        const int op = rd<int32_t>(), j = rd<int32_t>();
        if (op == 0) db.add(&kfs[j]); else db.erase(&kfs[j]);
    }
    for (int q = 0; q < n_q; q++) {
        const int mode = rd<int32_t>(), id = rd<int32_t>();
        BowVector bow;
        read_bow(bow);
        const float min_score = rd<float>();
        std::vector<uint8_t> conn(n_kf);
        for (int j = 0; j < n_kf; j++) conn[j] = rd<uint8_t>();
        for (int j = 0; j < n_kf; j++) { const float s = db.member(&kfs[j], mode); std::fwrite(&s, 4, 1, fo); }
        std::vector<KeyFrame*> got;
        if (mode == 0) {
            Frame F;
            F.mnId = id; F.mBowVec = bow;
            got = db.DetectRelocalizationCandidates(&F);
        } else {
            KeyFrame K;
            K.mnId = id; K.mBowVec = bow;
            for (int j = 0; j < n_kf; j++) if (conn[j]) K.connected.insert(&kfs[j]);
            got = db.DetectLoopCandidates(&K, min_score);
        }
        const int32_t nc = (int32_t)got.size();
        std::fwrite(&nc, 4, 1, fo);
        for (KeyFrame* k : got) { const int32_t s = (int32_t)(k - &kfs[0]); std::fwrite(&s, 4, 1, fo); }
        for (int j = 0; j < n_kf; j++) { const float s = db.member(&kfs[j], mode); std::fwrite(&s, 4, 1, fo); }
    }
    db.clear();
    Frame F;
    F.mBowVec = kfs[0].mBowVec;
    const int32_t after_clear = (int32_t)db.DetectRelocalizationCandidates(&F).size();
    std::fwrite(&after_clear, 4, 1, fo);
    std::fclose(fo);
    return 0;
}
