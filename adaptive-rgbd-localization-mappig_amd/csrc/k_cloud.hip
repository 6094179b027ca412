// Dense clouds for the frames of a batch at once: Frame::CreateCloud
// (Core/frame.cpp:191-215), Frame::VoxelGridFilterCloud (frame.cpp:217-226,
// pcl::VoxelGrid<PointXYZRGB> of PCL 1.8, restated: include/odo.h) and
// pcl::transformPointCloud (Tests/Draw_map_pose.cpp:72-73). A frame is never
// materialised as a cloud: a point is recomputed from its depth pixel wherever
// it is needed (three multiplies), so the scratch holds only (key, pixel) pairs.
//
// A frame's elements are cut into chunks of CLOUD_CHUNK = 1024, one wave per
// chunk, 16 rounds of 64 consecutive elements; a launch covers every chunk of
// every frame (grid.y = frame), so 256 frames are one chain of launches.
//
//   k_cloud_init     the frames' bounds to +-inf, their counts to 0
//   k_cloud_bounds   per chunk: valid pixels (z > 0) and the min / max of x, y,
//                    z as order-preserving integers (wave reduction, then
//                    integer atomics: exact in any order)
//   k_cloud_plan     one wave per frame: the exclusive scan of the chunks'
//                    valid counts, then VoxelGrid's min_b / div_b, its overflow
//                    return and the number of key bytes that can be set
//   k_cloud_keys     compaction in raster order (ballot / mbcnt) and the voxel
//                    key of every valid pixel (its position when unfiltered)
//   k_cloud_hist / _scan / _scatter   one stable LSD radix pass over 8 key bits:
//                    a 256-bin histogram per chunk, the exclusive scan in (bin,
//                    chunk) order, and the scatter, in which a lane's rank among
//                    the lanes of its round with the same digit comes from 8
//                    ballots. A frame skips the passes its div_b leaves zero.
//   k_cloud_heads    voxel heads (key != predecessor) per chunk
//   k_cloud_voxels   one wave per frame: scan of the chunks' head counts, n_points
//   k_cloud_offsets  the frames' offsets into the output
//   k_cloud_starts   every voxel's first sorted element (into the idle key buffer)
//   k_cloud_centroid 8 lanes per voxel: lane l adds the voxel's elements l, l + 8,
//                    ... in order, then a butterfly over the 8 lanes: a fixed
//                    order, so bit-identical run to run. Integer colour sums.
//                    The optional Twc and the 16-byte store.
#include "odo_device.h"
#include "odo_internal.h"
#include "odo_wave.h"

namespace odo {

#define CL_ROUNDS (CLOUD_CHUNK / 64)
#define CL_WAVES 4  // chunks (waves) per workgroup

// frame.cpp:200-205; false: the pixel has no point
ODO_INLINE bool cl_point(const uint16_t* __restrict__ D, int p, int W, const FrameCalib& k, float& x, float& y,
                         float& z) {
    z = (float)D[p] * k.depth_factor;
    const int i = p / W, j = p - i * W;
    x = ((float)j - k.cx) * z * k.invfx;
    y = ((float)i - k.cy) * z * k.invfy;
    return z > 0.0f;
}

// in-place exclusive scan of v[0..n) by one wave, 64 entries a round; returns the total
ODO_INLINE int cl_wave_scan(int32_t* __restrict__ v, int n, int lane) {
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane, t = c < n ? v[c] : 0;
        const int inc = wave_incl_scan_shfl(t, lane);
        if (c < n) v[c] = run + inc - t;
        run += __shfl(inc, 63);
    }
    return run;
}

__global__ void __launch_bounds__(256) k_cloud_init(CloudFrame* __restrict__ fr, int n) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    for (int a = 0; a < 3; a++) {
        fr[f].lo[a] = 0xffffffffu;
        fr[f].hi[a] = 0u;
    }
    fr[f].n_valid = 0;
}

__global__ void __launch_bounds__(256) k_cloud_bounds(const uint16_t* __restrict__ depth, int W, int P, int nch,
                                                      FrameCalib cal, CloudFrame* __restrict__ fr,
                                                      int32_t* __restrict__ chunk_off) {
    const int lane = threadIdx.x & 63, chunk = blockIdx.x * CL_WAVES + (threadIdx.x >> 6), f = blockIdx.y;
    if (chunk >= nch) return;
    const uint16_t* D = depth + (size_t)f * P;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    int cnt = 0;
    for (int r = 0; r < CL_ROUNDS; r++) {
        const int p = chunk * CLOUD_CHUNK + r * 64 + lane;
        float v[3];
        if (p < P && cl_point(D, p, W, cal, v[0], v[1], v[2])) {
            cnt++;
            for (int a = 0; a < 3; a++) {
                const uint32_t o = f32_ordered(v[a]);
                lo[a] = min(lo[a], o);
                hi[a] = max(hi[a], o);
            }
        }
    }
    for (int o = 32; o; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        for (int a = 0; a < 3; a++) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o));
        }
    }
    if (lane == 0) {
        chunk_off[(size_t)f * nch + chunk] = cnt;
        if (cnt) {
            atomicAdd(&fr[f].n_valid, cnt);
            for (int a = 0; a < 3; a++) {
                atomicMin(&fr[f].lo[a], lo[a]);
                atomicMax(&fr[f].hi[a], hi[a]);
            }
        }
    }
}

// key bytes that can be non-zero when every key is <= maxkey
ODO_INLINE int cl_key_bytes(uint32_t maxkey) { return maxkey == 0 ? 0 : maxkey < (1u << 8) ? 1 : maxkey < (1u << 16) ? 2 : maxkey < (1u << 24) ? 3 : 4; }

__global__ void __launch_bounds__(256) k_cloud_plan(CloudFrame* __restrict__ fr, odo_cloud_info* __restrict__ info,
                                                    int32_t* __restrict__ chunk_off, int n, int nch, float leaf) {
    // a wave per frame: its lanes scan the chunks' counts, lane 0 plans
    const int lane = threadIdx.x & 63, f = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (f >= n) return;
    cl_wave_scan(chunk_off + (size_t)f * nch, nch, lane);
    if (lane) return;
    CloudFrame F = fr[f];
    odo_cloud_info I;
    I.status = ODO_CLOUD_OK;
    I.n_valid = F.n_valid;
    I.n_points = 0;
    for (int a = 0; a < 3; a++) {
        I.min_b[a] = I.div_b[a] = 0;
        I.min_p[a] = I.max_p[a] = 0.0f;
        F.min_b[a] = 0;
    }
    F.filtered = 0;
    F.npass = 0;
    F.inv = 0.0f;
    F.div0 = F.div01 = 0u;
    F.n_points = F.out_off = 0;
    F.pad = 0;
    if (F.n_valid > 0) {
        for (int a = 0; a < 3; a++) {
            I.min_p[a] = f32_unordered(F.lo[a]);
            I.max_p[a] = f32_unordered(F.hi[a]);
        }
        bool ok = leaf > 0.0f;
        if (ok) {
            // applyFilter's "leaf size is too small" test (dx * dy * dz > INT32_MAX); a product that
            // no int64 holds is that return too
            const float inv = 1.0f / leaf;
            long long d[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++) {
                const float t = (I.max_p[a] - I.min_p[a]) * inv;
                if (!(t < 2147483648.0f)) ok = false;  // also NaN (0 * inf)
                else d[a] = (long long)t + 1;
            }
            if (ok && (d[0] * d[1] > 2147483647LL || d[0] * d[1] * d[2] > 2147483647LL)) ok = false;
            long long dv[3] = {0, 0, 0};
            int mb[3] = {0, 0, 0};
            if (ok)
                for (int a = 0; a < 3; a++) {
                    // min_b_ / max_b_ / div_b_; a floor outside int32 (undefined there) is the overflow return
                    const float fl = floorf(I.min_p[a] * inv), fh = floorf(I.max_p[a] * inv);
                    if (!(fl >= -2147483648.0f && fh < 2147483648.0f)) {
                        ok = false;
                        continue;
                    }
                    mb[a] = (int)fl;
                    dv[a] = (long long)(int)fh - mb[a] + 1;
                    if (dv[a] > 2147483647LL) ok = false;
                }
            if (ok) {
                F.filtered = 1;
                F.inv = inv;
                for (int a = 0; a < 3; a++) {
                    F.min_b[a] = I.min_b[a] = mb[a];
                    I.div_b[a] = (int)dv[a];
                }
                F.div0 = (uint32_t)dv[0];
                F.div01 = (uint32_t)dv[0] * (uint32_t)dv[1];
                // every key is below div_b's product where that fits 32 bits and
                // no axis is long enough for the float subtraction to round
                const double prod = (double)dv[0] * (double)dv[1] * (double)dv[2];
                const bool bounded = prod <= 4294967296.0 && dv[0] <= (1 << 24) && dv[1] <= (1 << 24) && dv[2] <= (1 << 24);
                F.npass = bounded ? cl_key_bytes((uint32_t)(prod - 1.0)) : 4;
            }
        }
        if (!F.filtered) I.status = ODO_CLOUD_UNFILTERED;
    }
    fr[f] = F;
    info[f] = I;
}

__global__ void __launch_bounds__(256) k_cloud_keys(const uint16_t* __restrict__ depth, int W, int P, int nch,
                                                    FrameCalib cal, const CloudFrame* __restrict__ fr,
                                                    const int32_t* __restrict__ chunk_off, uint32_t* __restrict__ key,
                                                    uint32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63, chunk = blockIdx.x * CL_WAVES + (threadIdx.x >> 6), f = blockIdx.y;
    if (chunk >= nch) return;
    const CloudFrame& F = fr[f];
    const uint16_t* D = depth + (size_t)f * P;
    uint32_t* K = key + (size_t)f * P;
    uint32_t* X = idx + (size_t)f * P;
    const bool filtered = F.filtered != 0;
    const float inv = F.inv, b0 = (float)F.min_b[0], b1 = (float)F.min_b[1], b2 = (float)F.min_b[2];
    const uint32_t div0 = F.div0, div01 = F.div01;
    int base = chunk_off[(size_t)f * nch + chunk];
    for (int r = 0; r < CL_ROUNDS; r++) {
        const int p = chunk * CLOUD_CHUNK + r * 64 + lane;
        float x = 0.f, y = 0.f, z = 0.f;
        const bool valid = p < P && cl_point(D, p, W, cal, x, y, z);
        const uint64_t m = __ballot(valid);
        const int pos = base + lane_rank(m);
        base += __popcll(m);
        if (valid) {
            uint32_t k = (uint32_t)pos;
            if (filtered) {
                // applyFilter's index vector
                const int i0 = (int)(floorf(x * inv) - b0), i1 = (int)(floorf(y * inv) - b1), i2 = (int)(floorf(z * inv) - b2);
                k = (uint32_t)i0 + (uint32_t)i1 * div0 + (uint32_t)i2 * div01;
            }
            K[pos] = k;
            X[pos] = (uint32_t)p;
        }
    }
}

__global__ void __launch_bounds__(256) k_cloud_hist(const CloudFrame* __restrict__ fr, const uint32_t* __restrict__ key0,
                                                    const uint32_t* __restrict__ key1, int32_t* __restrict__ hist, int P,
                                                    int nch, int pass) {
    __shared__ int s_cnt[CL_WAVES][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, chunk = blockIdx.x * CL_WAVES + w, f = blockIdx.y;
    const int nv = fr[f].n_valid;
    if (fr[f].npass <= pass || blockIdx.x * CL_WAVES * CLOUD_CHUNK >= nv) return;  // the whole workgroup
    const uint32_t* K = ((pass & 1) ? key1 : key0) + (size_t)f * P;
    for (int q = lane; q < 256; q += 64) s_cnt[w][q] = 0;
    __syncthreads();
    for (int r = 0; r < CL_ROUNDS; r++) {
        const int e = chunk * CLOUD_CHUNK + r * 64 + lane;
        if (e < nv) atomicAdd(&s_cnt[w][(K[e] >> (8 * pass)) & 255u], 1);
    }
    __syncthreads();
    if (chunk < nch && chunk * CLOUD_CHUNK < nv)
        for (int q = lane; q < 256; q += 64) hist[((size_t)f * nch + chunk) * 256 + q] = s_cnt[w][q];
}

// exclusive scan of a frame's histograms in (bin, chunk) order, in place: thread
// (g, t) adds bin t over the g-th quarter of the chunks, the bins' totals are
// scanned, and each quarter is rewritten from its own start
#define CL_SCAN_GROUPS 4
__global__ void __launch_bounds__(256 * CL_SCAN_GROUPS) k_cloud_scan(const CloudFrame* __restrict__ fr,
                                                                     int32_t* __restrict__ hist, int nch, int pass) {
    __shared__ int s_part[CL_SCAN_GROUPS][256];
    __shared__ int s_tot[256];
    const int f = blockIdx.x, t = threadIdx.x & 255, g = threadIdx.x >> 8;
    if (fr[f].npass <= pass) return;
    const int used = (fr[f].n_valid + CLOUD_CHUNK - 1) / CLOUD_CHUNK, per = (used + CL_SCAN_GROUPS - 1) / CL_SCAN_GROUPS;
    const int c0 = min(g * per, used), c1 = min(c0 + per, used);
    int32_t* Hf = hist + (size_t)f * nch * 256;
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += Hf[(size_t)c * 256 + t];
    s_part[g][t] = sum;
    __syncthreads();
    int before = 0, tot = 0;
    for (int q = 0; q < CL_SCAN_GROUPS; q++) {
        const int v = s_part[q][t];
        if (q < g) before += v;
        tot += v;
    }
    if (g == 0) s_tot[t] = tot;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = (g == 0 && t >= o) ? s_tot[t - o] : 0;
        __syncthreads();
        if (g == 0) s_tot[t] += v;
        __syncthreads();
    }
    int run = s_tot[t] - tot + before;
    for (int c = c0; c < c1; c++) {
        const int v = Hf[(size_t)c * 256 + t];
        Hf[(size_t)c * 256 + t] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(256) k_cloud_scatter(const CloudFrame* __restrict__ fr, uint32_t* __restrict__ key0,
                                                       uint32_t* __restrict__ key1, uint32_t* __restrict__ idx0,
                                                       uint32_t* __restrict__ idx1, const int32_t* __restrict__ hist,
                                                       int P, int nch, int pass) {
    __shared__ int s_off[CL_WAVES][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, chunk = blockIdx.x * CL_WAVES + w, f = blockIdx.y;
    const int nv = fr[f].n_valid;
    if (fr[f].npass <= pass || blockIdx.x * CL_WAVES * CLOUD_CHUNK >= nv) return;  // the whole workgroup
    const size_t fo = (size_t)f * P;
    const uint32_t *K = ((pass & 1) ? key1 : key0) + fo, *X = ((pass & 1) ? idx1 : idx0) + fo;
    uint32_t *Kd = ((pass & 1) ? key0 : key1) + fo, *Xd = ((pass & 1) ? idx0 : idx1) + fo;
    const bool live = chunk < nch && chunk * CLOUD_CHUNK < nv;
    for (int q = lane; q < 256; q += 64) s_off[w][q] = live ? hist[((size_t)f * nch + chunk) * 256 + q] : 0;
    __syncthreads();
    for (int r = 0; r < CL_ROUNDS; r++) {
        const int e = chunk * CLOUD_CHUNK + r * 64 + lane;
        const bool valid = live && e < nv;
        const uint32_t k = valid ? K[e] : 0u, x = valid ? X[e] : 0u;
        const uint32_t d = (k >> (8 * pass)) & 255u;
        // the valid lanes of this round with the same digit
        uint64_t m = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bb = __ballot(bit);
            m &= bit ? bb : ~bb;
        }
        const int rank = lane_rank(m);
        const int off = valid ? s_off[w][d] : 0;
        __syncthreads();
        if (valid && rank == 0) s_off[w][d] = off + __popcll(m);
        __syncthreads();
        if (valid) {
            Kd[off + rank] = k;
            Xd[off + rank] = x;
        }
    }
}

__global__ void __launch_bounds__(256) k_cloud_heads(const CloudFrame* __restrict__ fr, const uint32_t* __restrict__ key0,
                                                     const uint32_t* __restrict__ key1, int32_t* __restrict__ head_off,
                                                     int P, int nch) {
    const int lane = threadIdx.x & 63, chunk = blockIdx.x * CL_WAVES + (threadIdx.x >> 6), f = blockIdx.y;
    if (chunk >= nch) return;
    const int nv = fr[f].n_valid;
    const uint32_t* K = ((fr[f].npass & 1) ? key1 : key0) + (size_t)f * P;
    int cnt = 0;
    if (chunk * CLOUD_CHUNK < nv)
        for (int r = 0; r < CL_ROUNDS; r++) {
            const int e = chunk * CLOUD_CHUNK + r * 64 + lane;
            const bool head = e < nv && (e == 0 || K[e] != K[e - 1]);
            cnt += __popcll(__ballot(head));
        }
    if (lane == 0) head_off[(size_t)f * nch + chunk] = cnt;
}

__global__ void __launch_bounds__(256) k_cloud_voxels(CloudFrame* __restrict__ fr, odo_cloud_info* __restrict__ info,
                                                      int32_t* __restrict__ head_off, int n, int nch) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (f >= n) return;
    const int np = cl_wave_scan(head_off + (size_t)f * nch, nch, lane);
    if (lane == 0) {
        fr[f].n_points = np;
        info[f].n_points = np;
    }
}

// the frames' first points: one wave, the frames in order
__global__ void __launch_bounds__(64) k_cloud_offsets(CloudFrame* __restrict__ fr, int n) {
    const int lane = threadIdx.x;
    int run = 0;
    for (int f0 = 0; f0 < n; f0 += 64) {
        const int f = f0 + lane, t = f < n ? fr[f].n_points : 0;
        const int inc = wave_incl_scan_shfl(t, lane);
        if (f < n) fr[f].out_off = run + inc - t;
        run += __shfl(inc, 63);
    }
}

__global__ void __launch_bounds__(256) k_cloud_starts(const CloudFrame* __restrict__ fr, uint32_t* __restrict__ key0,
                                                      uint32_t* __restrict__ key1, const int32_t* __restrict__ head_off,
                                                      int P, int nch) {
    const int lane = threadIdx.x & 63, chunk = blockIdx.x * CL_WAVES + (threadIdx.x >> 6), f = blockIdx.y;
    if (chunk >= nch) return;
    const int nv = fr[f].n_valid;
    if (chunk * CLOUD_CHUNK >= nv) return;
    const bool odd = fr[f].npass & 1;
    const uint32_t* K = (odd ? key1 : key0) + (size_t)f * P;
    uint32_t* V = (odd ? key0 : key1) + (size_t)f * P;
    int base = head_off[(size_t)f * nch + chunk];
    for (int r = 0; r < CL_ROUNDS; r++) {
        const int e = chunk * CLOUD_CHUNK + r * 64 + lane;
        const bool head = e < nv && (e == 0 || K[e] != K[e - 1]);
        const uint64_t m = __ballot(head);
        if (head) V[base + lane_rank(m)] = (uint32_t)e;
        base += __popcll(m);
    }
}

#define CL_GROUP 8  // lanes per voxel
__global__ void __launch_bounds__(256) k_cloud_centroid(const uint8_t* __restrict__ bgr, const uint16_t* __restrict__ depth,
                                                        int W, int P, FrameCalib cal, const CloudFrame* __restrict__ fr,
                                                        const uint32_t* __restrict__ key0, const uint32_t* __restrict__ key1,
                                                        const uint32_t* __restrict__ idx0, const uint32_t* __restrict__ idx1,
                                                        const float* __restrict__ Twc, odo_cloud_point* __restrict__ out,
                                                        int32_t* __restrict__ counts) {
    const int f = blockIdx.y, sub = threadIdx.x & (CL_GROUP - 1);
    const int v = blockIdx.x * (256 / CL_GROUP) + (threadIdx.x / CL_GROUP);
    const CloudFrame& F = fr[f];
    const int np = F.n_points, nv = F.n_valid;
    const bool odd = F.npass & 1, live = v < np;
    const uint32_t* V = (odd ? key0 : key1) + (size_t)f * P;
    const uint32_t* X = (odd ? idx1 : idx0) + (size_t)f * P;
    const uint16_t* D = depth + (size_t)f * P;
    const uint8_t* C = bgr + (size_t)f * P * 3;
    int e0 = 0, e1 = 0;
    if (live) {
        e0 = (int)V[v];
        e1 = v + 1 < np ? (int)V[v + 1] : nv;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f;
    uint32_t sb = 0, sg = 0, sr = 0;
    for (int e = e0 + sub; e < e1; e += CL_GROUP) {
        const int p = (int)X[e];
        float x, y, z;
        cl_point(D, p, W, cal, x, y, z);
        sx += x;
        sy += y;
        sz += z;
        sb += C[3 * (size_t)p];
        sg += C[3 * (size_t)p + 1];
        sr += C[3 * (size_t)p + 2];
    }
    for (int o = CL_GROUP / 2; o; o >>= 1) {
        sx += __shfl_xor(sx, o);
        sy += __shfl_xor(sy, o);
        sz += __shfl_xor(sz, o);
        sb += (uint32_t)__shfl_xor((int)sb, o);
        sg += (uint32_t)__shfl_xor((int)sg, o);
        sr += (uint32_t)__shfl_xor((int)sr, o);
    }
    if (!live || sub) return;
    const int cnt = e1 - e0;
    const float fc = (float)cnt;
    float x = sx / fc, y = sy / fc, z = sz / fc;
    // the colour channels (and a, 255 at every point) are averaged like the coordinates
    const uint32_t b = (uint32_t)((float)sb / fc) & 255u, g = (uint32_t)((float)sg / fc) & 255u,
                   r = (uint32_t)((float)sr / fc) & 255u, al = (uint32_t)((float)(255u * (uint32_t)cnt) / fc) & 255u;
    if (Twc) {
        const float* M = Twc + (size_t)f * 16;
        const float tx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
        const float ty = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
        const float tz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
        x = tx;
        y = ty;
        z = tz;
    }
    const size_t o = (size_t)F.out_off + v;
    uint4 q;
    q.x = __float_as_uint(x);
    q.y = __float_as_uint(y);
    q.z = __float_as_uint(z);
    q.w = b | (g << 8) | (r << 16) | (al << 24);
    *reinterpret_cast<uint4*>(out + o) = q;
    counts[o] = cnt;
}

void launch_cloud_voxels(hipStream_t st, const CloudArgs& a) {
    const int P = a.W * a.H;
    const dim3 grid((a.nch + CL_WAVES - 1) / CL_WAVES, a.n), blk(256);
    hipLaunchKernelGGL(k_cloud_init, dim3((a.n + 255) / 256), blk, 0, st, a.fr, a.n);
    hipLaunchKernelGGL(k_cloud_bounds, grid, blk, 0, st, a.depth, a.W, P, a.nch, a.cal, a.fr, a.chunk_off);
    hipLaunchKernelGGL(k_cloud_plan, dim3((a.n + CL_WAVES - 1) / CL_WAVES), blk, 0, st, a.fr, a.info, a.chunk_off, a.n, a.nch, a.leaf);
    hipLaunchKernelGGL(k_cloud_keys, grid, blk, 0, st, a.depth, a.W, P, a.nch, a.cal, a.fr, a.chunk_off, a.key[0], a.idx[0]);
    if (a.leaf > 0.0f)  // an unfiltered call has no frame with a pass
        for (int pass = 0; pass < 4; pass++) {
            hipLaunchKernelGGL(k_cloud_hist, grid, blk, 0, st, a.fr, a.key[0], a.key[1], a.hist, P, a.nch, pass);
            hipLaunchKernelGGL(k_cloud_scan, dim3(a.n), dim3(256 * CL_SCAN_GROUPS), 0, st, a.fr, a.hist, a.nch, pass);
            hipLaunchKernelGGL(k_cloud_scatter, grid, blk, 0, st, a.fr, a.key[0], a.key[1], a.idx[0], a.idx[1], a.hist, P,
                               a.nch, pass);
        }
    hipLaunchKernelGGL(k_cloud_heads, grid, blk, 0, st, a.fr, a.key[0], a.key[1], a.head_off, P, a.nch);
    hipLaunchKernelGGL(k_cloud_voxels, dim3((a.n + CL_WAVES - 1) / CL_WAVES), blk, 0, st, a.fr, a.info, a.head_off, a.n,
                       a.nch);
    hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(64), 0, st, a.fr, a.n);
}

void launch_cloud_points(hipStream_t st, const CloudArgs& a, int max_points) {
    if (max_points <= 0) return;
    const int P = a.W * a.H;
    const dim3 grid((a.nch + CL_WAVES - 1) / CL_WAVES, a.n), blk(256);
    hipLaunchKernelGGL(k_cloud_starts, grid, blk, 0, st, a.fr, a.key[0], a.key[1], a.head_off, P, a.nch);
    const int per = 256 / CL_GROUP;
    hipLaunchKernelGGL(k_cloud_centroid, dim3((max_points + per - 1) / per, a.n), blk, 0, st, a.bgr, a.depth, a.W, P, a.cal,
                       a.fr, a.key[0], a.key[1], a.idx[0], a.idx[1], a.Twc, a.out, a.counts);
}

}  // namespace odo
