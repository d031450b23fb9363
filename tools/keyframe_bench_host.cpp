// tools/keyframe_bench_host.cpp — the host side of tools/keyframe_bench.py: the end of Tracking::Track with NeedNewKeyFrame, CreateNewKeyFrame and the head of
// ProcessNewKeyFrame restated over the arrays of ONE map of planar_map_edit and ONE frame, run by ONE thread (compiled -O2 by the tool).  The tool's batches hold
// the same frame and the same map B or G times, so a batch costs B or G times what is timed here on private copies.
// Input (int32 stream, floats as bits): S SS PS OC nk npts reps N th; kf_rank [S], n_slots [S], kf_pts [S][SS], pt_bad [PS], pt_nobs [PS], obs_off [PS + 1],
// obs_kf [OC]; match [N], outlier [N], depth [N], u_right [N]; ref_kf, nKFs, frame_id, last_kf, max_frames, min_frames, flags.
// Output (int32 stream): need microseconds [reps], create + add microseconds [reps], then need, inliers, n_ref, n_map, n_total, created, added of the last one.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

static float as_float(int32_t v) { float f; memcpy(&f, &v, 4); return f; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<int32_t> in(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    const int32_t* p = in.data();
    const int S = p[0], SS = p[1], PS = p[2], OC = p[3], nk = p[4], npts = p[5], reps = p[6], N = p[7];
    const float th = as_float(p[8]);
    p += 9;
    const int32_t* rank0 = p; p += S;
    const int32_t* n_slots0 = p; p += S;
    const int32_t* kf_pts0 = p; p += (size_t)S * SS;
    const int32_t* pt_bad0 = p; p += PS;
    const int32_t* pt_nobs0 = p; p += PS;
    const int32_t* obs_off0 = p; p += PS + 1;
    const int32_t* obs_kf0 = p; p += OC;
    const int32_t* match0 = p; p += N;
    const int32_t* outl0 = p; p += N;
    const int32_t* depth = p; p += N;
    const int32_t* uright = p; p += N;
    const int ref_kf = p[0], nKFs = p[1], frame_id = p[2], last_kf = p[3], max_frames = p[4], min_frames = p[5], flags = p[6];
    std::vector<int32_t> out, t_need, t_grow, last;
    for (int rep = 0; rep < reps; rep++) {
        std::vector<int32_t> rank(rank0, rank0 + S), n_slots(n_slots0, n_slots0 + S), kf_pts(kf_pts0, kf_pts0 + (size_t)S * SS), pt_bad(pt_bad0, pt_bad0 + PS),
            pt_nobs(pt_nobs0, pt_nobs0 + PS), obs_off(obs_off0, obs_off0 + PS + 1), obs_kf(obs_kf0, obs_kf0 + OC), match(match0, match0 + N), outl(outl0, outl0 + N);
        // ---- count, clean, decide
        auto t0 = std::chrono::steady_clock::now();
        int inl = 0;
        for (int i = 0; i < N; i++)
            if (match[i] >= 0 && !outl[i] && ((flags & 1) || pt_nobs[match[i]] > 0)) inl++;
        for (int i = 0; i < N; i++)
            if (match[i] >= 0 && pt_nobs[match[i]] < 1) { outl[i] = 0; match[i] = -1; }
        const int nMinObs = nKFs <= 2 ? 2 : 3;
        int nref = 0, nmap = 0, ntot = 0;
        for (int s = 0; s < n_slots[ref_kf]; s++) {
            const int q = kf_pts[(size_t)ref_kf * SS + s];
            if (q >= 0 && !pt_bad[q] && pt_nobs[q] >= nMinObs) nref++;
        }
        for (int i = 0; i < N; i++) {
            const float z = as_float(depth[i]);
            if (z > 0 && z < th) { ntot++; if (match[i] >= 0 && !outl[i]) nmap++; }
        }
        const bool idle = (flags & 4) != 0;
        const float ratio = (float)nmap / fmax(1.0f, ntot);
        const float thRef = nKFs < 2 ? 0.4f : 0.75f, thMap = inl > 300 ? 0.20f : 0.35f;
        const bool c1a = frame_id >= last_kf + max_frames, c1b = frame_id >= last_kf + min_frames && idle, c1c = inl < nref * 0.25 || ratio < 0.3f;
        const bool c2 = (inl < nref * thRef || ratio < thMap) && inl > 15;
        const int need = !(flags & 3) && (((c1a || c1b || c1c) && c2) || (flags & 8)) && idle;
        auto t1 = std::chrono::steady_clock::now();
        t_need.push_back((int32_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
        // ---- create and add
        t0 = std::chrono::steady_clock::now();
        std::vector<std::pair<float, int>> v;
        for (int i = 0; i < N; i++) { const float z = as_float(depth[i]); if (z > 0) v.push_back({z, i}); }
        std::sort(v.begin(), v.end());
        const int k = nk;
        int np = npts, used = obs_off[npts], created = 0, n = 0;
        for (int x = 0; x < nk; x++) if (rank[x] >= nk) rank[x]++;
        rank[k] = nk; n_slots[k] = N;
        std::copy(match.begin(), match.end(), kf_pts.begin() + (size_t)k * SS);
        for (size_t j = 0; j < v.size(); j++) {
            const int i = v[j].second, m = match[i];
            if (m < 0 || pt_nobs[m] < 1) {
                pt_bad[np] = 0; pt_nobs[np] = as_float(uright[i]) >= 0 ? 2 : 1; obs_kf[used] = k; obs_off[np + 1] = ++used;
                kf_pts[(size_t)k * SS + i] = np; match[i] = np; np++; created++;
            }
            n++;
            if (v[j].first > th && n > 100) break;
        }
        // the observation lists with the new key frame inserted where it belongs: one pass over the CSR
        std::vector<int32_t> first(np, -1), new_kf((size_t)OC), new_off(np + 1);
        int added = 0;
        for (int i = 0; i < N; i++) {
            const int q = kf_pts[(size_t)k * SS + i];
            if (q < 0 || pt_bad[q] || first[q] >= 0) continue;
            bool listed = false;
            for (int o = obs_off[q]; o < obs_off[q + 1]; o++) listed |= obs_kf[o] == k;
            if (!listed) first[q] = i;
        }
        int at = 0;
        for (int q = 0; q < np; q++) {
            new_off[q] = at;
            int o = obs_off[q];
            if (first[q] >= 0) {
                for (; o < obs_off[q + 1] && rank[obs_kf[o]] < rank[k]; o++) new_kf[at++] = obs_kf[o];
                new_kf[at++] = k; pt_nobs[q] += as_float(uright[first[q]]) >= 0 ? 2 : 1; added++;
            }
            for (; o < obs_off[q + 1]; o++) new_kf[at++] = obs_kf[o];
        }
        new_off[np] = at;
        obs_kf.swap(new_kf); std::copy(new_off.begin(), new_off.end(), obs_off.begin());
        t1 = std::chrono::steady_clock::now();
        t_grow.push_back((int32_t)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count());
        last = {need, inl, nref, nmap, ntot, created, added};
    }
    out.insert(out.end(), t_need.begin(), t_need.end());
    out.insert(out.end(), t_grow.begin(), t_grow.end());
    out.insert(out.end(), last.begin(), last.end());
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
