// tools/kfdb_golden/ref_kfdb_main.cpp — TEST INFRASTRUCTURE.  Driver of the REAL KeyFrameDatabase (src/KeyFrameDatabase.cc) and DBoW2 vocabulary for
// tools/gen_golden_kfdb.py:   ref_kfdb <vocabulary.txt> <in.bin> <out.bin>
// in.bin : int32 n_kf, n_ops, n_q, n_pairs; per key frame int32 n, n x int32 word, n x double value, 10 x int32 covisible slot (-1: none);
//          n_ops x {int32 op (0 add, 1 erase), int32 slot}; per query int32 mode (0 reloc, 1 loop), int32 mnId, int32 n, words, values, float minScore,
//          n_kf x uint8 connected; n_pairs x {int32 a, int32 b} (index < n_kf: key frame, else query) for Vocabulary::score.
// The queries run one after the other on the same KeyFrame objects.
// out.bin: per query n_kf x float the key frames' mRelocScore / mLoopScore BEFORE the query, int32 n_cand, n_cand x int32 slot of the returned vector,
//          n_kf x int32 mnRelocWords / mnLoopWords where mnRelocQuery / mnLoopQuery is the query's id (0 elsewhere), n_kf x float the scores after the query,
//          int32 nscores (a local of the reference: counted here as the marked key frames above (int)(max words * 0.8f)); then n_pairs x double.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "KeyFrameDatabase.h"

using namespace Planar_SLAM;

static FILE* fi;
template <typename T> static T rd() { T v; if (std::fread(&v, sizeof(T), 1, fi) != 1) std::exit(4); return v; }
static void read_bow(DBoW2::BowVector& v) {
    const int n = rd<int32_t>();
    std::vector<int32_t> w(n);
    for (int i = 0; i < n; i++) w[i] = rd<int32_t>();
    for (int i = 0; i < n; i++) v.insert(std::make_pair((DBoW2::WordId)w[i], rd<double>()));
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) return 3;
    fi = std::fopen(argv[2], "rb");
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fi || !fo) return 2;
    const int n_kf = rd<int32_t>(), n_ops = rd<int32_t>(), n_q = rd<int32_t>(), n_pairs = rd<int32_t>();
    std::vector<KeyFrame> kfs(n_kf);
    std::vector<std::vector<int32_t>> cov(n_kf, std::vector<int32_t>(10));
    for (int j = 0; j < n_kf; j++) {
        kfs[j].mnId = j + 1;
        read_bow(kfs[j].mBowVec);
        for (int t = 0; t < 10; t++) cov[j][t] = rd<int32_t>();
    }
    for (int j = 0; j < n_kf; j++)
        for (int t = 0; t < 10; t++) if (cov[j][t] >= 0) kfs[j].covisible.push_back(&kfs[cov[j][t]]);
    KeyFrameDatabase db(voc);
    for (int i = 0; i < n_ops; i++) {
        const int op = rd<int32_t>(), j = rd<int32_t>();
        if (op == 0) db.add(&kfs[j]); else db.erase(&kfs[j]);
    }
    std::vector<DBoW2::BowVector> qbow(n_q);
    for (int q = 0; q < n_q; q++) {
        const int mode = rd<int32_t>(), id = rd<int32_t>();
        read_bow(qbow[q]);
        const float min_score = rd<float>();
        std::vector<uint8_t> conn(n_kf);
        for (int j = 0; j < n_kf; j++) conn[j] = rd<uint8_t>();
        for (int j = 0; j < n_kf; j++) { const float s = mode ? kfs[j].mLoopScore : kfs[j].mRelocScore; std::fwrite(&s, 4, 1, fo); }
        std::vector<KeyFrame*> got;
        if (mode == 0) {
            Frame F;
            F.mnId = id; F.mBowVec = qbow[q];
            got = db.DetectRelocalizationCandidates(&F);
        } else {
            KeyFrame K;
            K.mnId = id; K.mBowVec = qbow[q];
            for (int j = 0; j < n_kf; j++) if (conn[j]) K.connected.insert(&kfs[j]);
            got = db.DetectLoopCandidates(&K, min_score);
        }
        const int32_t nc = (int32_t)got.size();
        std::fwrite(&nc, 4, 1, fo);
        for (KeyFrame* k : got) { const int32_t s = (int32_t)(k - &kfs[0]); std::fwrite(&s, 4, 1, fo); }
        int max_words = 0;
        std::vector<int32_t> words(n_kf, 0);
        for (int j = 0; j < n_kf; j++) {
            const bool marked = (mode ? kfs[j].mnLoopQuery : kfs[j].mnRelocQuery) == (long unsigned int)id;
            words[j] = marked ? (mode ? kfs[j].mnLoopWords : kfs[j].mnRelocWords) : 0;
            if (words[j] > max_words) max_words = words[j];
        }
        std::fwrite(words.data(), 4, n_kf, fo);
        for (int j = 0; j < n_kf; j++) { const float s = mode ? kfs[j].mLoopScore : kfs[j].mRelocScore; std::fwrite(&s, 4, 1, fo); }
        const int min_words = max_words * 0.8f;
        int32_t nscores = 0;
        for (int j = 0; j < n_kf; j++) nscores += words[j] > min_words;
        std::fwrite(&nscores, 4, 1, fo);
    }
    for (int p = 0; p < n_pairs; p++) {
        const int a = rd<int32_t>(), b = rd<int32_t>();
        const double s = voc.score(a < n_kf ? kfs[a].mBowVec : qbow[a - n_kf], b < n_kf ? kfs[b].mBowVec : qbow[b - n_kf]);
        std::fwrite(&s, 8, 1, fo);
    }
    std::fclose(fo);
    return 0;
}
