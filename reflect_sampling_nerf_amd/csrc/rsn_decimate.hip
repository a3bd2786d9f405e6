// Vertex-clustering decimation of an indexed triangle mesh (include/rsn.h, "decimation").
//
// One lane per vertex, per triangle, per cluster cell or per occupied cell, in grid-stride loops; every kernel is one pass.
//
//   cluster  (1) the cell of every vertex into the workspace, and a 1 into the cell's word of a dense occupancy array (plain
//            stores of one value: no atomic); (2) the occupancy array turns, in place, into the RANK of every occupied cell among
//            the occupied cells in ascending cell id, by the compaction of rsn_pointcloud_select -- counts of tiles of 256, one
//            workgroup that scans them (the one serial step: 256 tiles per iteration), placement by wave ballots; (3) the cell of
//            every vertex is replaced by that rank; (4) per triangle the 63-bit key of its three ranks in ascending order, its
//            orientation against that order, and the degenerate count.
//   resolve  the caller has sorted the keys stably: the lane at the first entry of a group walks the group (its triangles come in
//            ascending original index), counts the two orientations and flags the first |net| of the majority.  A group is as long
//            as the triangles that share three cells: a handful on a surface mesh, so the walk is short; a mesh of many copies of
//            one triangle walks them in one lane.
//   count    the cells the flagged triangles name, then two more compactions: triangle -> output row, rank -> output vertex.
//   emit     the fixed-point sums of every vertex of a named cell by 64-bit integer atomic adds (the feature's only atomics, with
//            the 32-bit counts: integer sums do not depend on the order), then the representatives and the renumbered triangles.
//            Neighbouring lanes often add to one cell (the extractor emits vertices in grid order); a pre-reduction of equal
//            neighbours inside a wave would keep the integer result and has not been tried or measured.
//
// Every fp32 step of the cell rule is one correctly rounded operation, spelled with __fsub_rn / __fdiv_rn / __fmul_rn so that none
// is contracted; the representative is fp64 (the library is built with -ffp-contract=off).  tests/test_decimate_gpu.py holds the
// calls to the bits of a numpy restatement.
#include "rsn_common.h"

#include <math.h>

#define RSN_DEC_BLOCK 256
#define RSN_DEC_MAX_BLOCKS 1024           // four workgroups per CU; past 262,144 items a workgroup walks several tiles
#define RSN_DEC_MAX_CELLS (1 << 27)       // the limit of the mesh, TSDF and point-cloud calls
#define RSN_DEC_MAX_OCCUPIED (1 << 21)    // three ranks of 21 bits in one sort key
#define RSN_DEC_NO_KEY 0x7fffffffffffffffLL
#define RSN_DEC_ONE 1048576.0f            // 2^20: the fixed-point unit of a position inside its cell

struct DecFrame {
  int n[3];
  float org[3], cel[3];
};

// The cell index of one coordinate and its fixed-point position inside the cell.
__device__ __forceinline__ int dec_axis(float p, float o, float c, int n, int* q) {
  float u = __fdiv_rn(__fsub_rn(p, o), c);
  if (!(fabsf(u) <= 3.402823466e38f)) u = 0.0f;                       // NaN and the infinities
  const float fl = fminf(fmaxf(floorf(u), 0.0f), 134217728.0f);       // 2^27: every integer up to it converts exactly
  const int i = min((int)fl, n - 1);
  const float f = __fsub_rn(u, (float)i);
  *q = (int)fminf(fmaxf(rintf(__fmul_rn(f, RSN_DEC_ONE)), 0.0f), RSN_DEC_ONE);  // ties to even; an infinite product clamps
  return i;
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_cell_kernel(const DecFrame f, int V, const float* __restrict__ pos,
                                                                          int* __restrict__ vert_cell, int* __restrict__ occ) {
  for (int64_t v = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    int idx[3], q;
#pragma unroll
    for (int a = 0; a < 3; ++a) idx[a] = dec_axis(pos[v * 3 + a], f.org[a], f.cel[a], f.n[a], &q);
    const int cell = (idx[2] * f.n[1] + idx[1]) * f.n[0] + idx[0];   // below 2^27
    vert_cell[v] = cell;
    occ[cell] = 1;
  }
}

// ---- the stable compaction of a flag array: src[i] != 0 -> dst[i] = the number of set flags in front of i, else -1
__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_tile_kernel(int n, int n_tiles, const int* __restrict__ src,
                                                                          int* __restrict__ tile_counts) {
  __shared__ int s_wave_tot[RSN_DEC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // the bound is the same in every lane
    const int64_t i = (int64_t)tile * RSN_DEC_BLOCK + tid;
    const bool set = i < n && src[i] != 0;
    const unsigned long long bal = __ballot(set);
    if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
    __syncthreads();
    if (tid == 0) {
      int t = 0;
#pragma unroll
      for (int wv = 0; wv < RSN_DEC_BLOCK / 64; ++wv) t += s_wave_tot[wv];
      tile_counts[tile] = t;
    }
    __syncthreads();  // s_wave_tot is read before the next tile writes it
  }
}

// One workgroup: counts[t] -> the number of set flags in the tiles in front of t (in place), their total -> *total.
__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_scan_kernel(int n_tiles, int* __restrict__ counts, int* __restrict__ total) {
  __shared__ int s_wave_tot[RSN_DEC_BLOCK / 64];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n_tiles; base += RSN_DEC_BLOCK) {  // the bound is the same in every lane
    const int j = base + tid;
    const int v = j < n_tiles ? counts[j] : 0;
    int x = v;  // inclusive scan of the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_wave_tot[wid] = x;
    __syncthreads();
    int wave_off = 0, tot = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_DEC_BLOCK / 64; ++wv) {
      const int t = s_wave_tot[wv];
      if (wv < wid) wave_off += t;
      tot += t;
    }
    const int carry = s_carry;
    if (j < n_tiles) counts[j] = carry + wave_off + x - v;
    __syncthreads();  // every lane has read s_carry and s_wave_tot
    if (tid == 0) s_carry = carry + tot;
    __syncthreads();
  }
  if (tid == 0) *total = s_carry;
}

// dst may be src.  inverse (or NULL): inverse[rank] = i for every set flag.
__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_place_kernel(int n, int n_tiles, const int* src, int* dst,
                                                                           const int* __restrict__ tile_offsets, int* __restrict__ inverse) {
  __shared__ int s_wave_tot[RSN_DEC_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t i = (int64_t)tile * RSN_DEC_BLOCK + tid;
    const bool set = i < n && src[i] != 0;
    const unsigned long long bal = __ballot(set);
    const int in_wave = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_tot[wid] = __builtin_popcountll(bal);
    __syncthreads();
    int wave_off = 0;
#pragma unroll
    for (int wv = 0; wv < RSN_DEC_BLOCK / 64; ++wv)
      if (wv < wid) wave_off += s_wave_tot[wv];
    if (i < n) {
      const int r = tile_offsets[tile] + wave_off + in_wave;
      dst[i] = set ? r : -1;
      if (set && inverse) inverse[r] = (int)i;
    }
    __syncthreads();  // s_wave_tot is read before the next tile writes it
  }
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_vert_rank_kernel(int V, int* __restrict__ vert, const int* __restrict__ rank) {
  for (int64_t v = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * RSN_DEC_BLOCK)
    vert[v] = rank[vert[v]];  // the cell of a vertex is occupied: a rank, never -1
}

// key, orientation and the cleared flag of every triangle; counts[2] += the degenerate ones.  counts[4] holds the occupied cells.
__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_key_kernel(int V, int T, const int* __restrict__ tri,
                                                                         const int* __restrict__ vert_rank, long long* __restrict__ keys,
                                                                         signed char* __restrict__ sign, int* __restrict__ keep,
                                                                         int* __restrict__ counts) {
  const bool overflow = counts[4] > RSN_DEC_MAX_OCCUPIED;  // the ranks do not fit the key: nothing is grouped or counted
  int degenerate = 0;
  for (int64_t t = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; t < T; t += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    const int a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    long long key = RSN_DEC_NO_KEY;
    signed char s = 0;
    if (!overflow) {
      bool live = (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;  // else nothing is dereferenced
      if (live) {
        const int ra = vert_rank[a], rb = vert_rank[b], rc = vert_rank[c];
        live = ra != rb && rb != rc && ra != rc;
        if (live) {
          const int lo = min(ra, min(rb, rc)), hi = max(ra, max(rb, rc)), mid = ra + rb + rc - lo - hi;
          key = ((long long)lo << 42) | ((long long)mid << 21) | (long long)hi;
          s = ((ra < rb) + (rb < rc) + (rc < ra)) == 2 ? 1 : -1;  // two ascents around the cycle: the cyclic order of the ascending cells
        }
      }
      degenerate += live ? 0 : 1;
    }
    keys[t] = key;
    sign[t] = s;
    keep[t] = 0;
  }
  if (degenerate) atomicAdd(counts + 2, degenerate);
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_resolve_kernel(int T, const long long* __restrict__ keys,
                                                                             const long long* __restrict__ order,
                                                                             const signed char* __restrict__ sign, int* __restrict__ keep,
                                                                             int* __restrict__ counts) {
  int survivors = 0, cancelled = 0;
  for (int64_t j = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; j < T; j += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    const long long key = keys[j];
    if (key == RSN_DEC_NO_KEY || (j > 0 && keys[j - 1] == key)) continue;  // degenerate, or not the first of its group
    int plus = 0, minus = 0;
    for (int64_t e = j; e < T && keys[e] == key; ++e) {
      const unsigned long long t = (unsigned long long)order[e];
      if (t >= (unsigned long long)T) continue;  // not an index: a caller's error, never dereferenced
      const int s = sign[t];
      plus += s > 0;
      minus += s < 0;
    }
    const int net = plus - minus, want = net > 0 ? 1 : -1;
    int left = net > 0 ? net : -net;
    survivors += left;
    cancelled += min(plus, minus);
    for (int64_t e = j; left > 0 && e < T && keys[e] == key; ++e) {
      const unsigned long long t = (unsigned long long)order[e];
      if (t >= (unsigned long long)T) continue;
      if (sign[t] == want) {
        keep[t] = 1;
        --left;
      }
    }
  }
  if (survivors) atomicAdd(counts + 1, survivors);
  if (cancelled) atomicAdd(counts + 3, cancelled);
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_used_kernel(int T, const int* __restrict__ tri, const int* __restrict__ keep,
                                                                          const int* __restrict__ vert_rank, int* __restrict__ used) {
  for (int64_t t = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; t < T; t += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    if (!keep[t]) continue;  // a kept triangle's indices are inside [0, V)
#pragma unroll
    for (int c = 0; c < 3; ++c) used[vert_rank[tri[t * 3 + c]]] = 1;
  }
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_sum_kernel(const DecFrame f, int V, const float* __restrict__ pos,
                                                                         const int* __restrict__ vert_rank, const int* __restrict__ new_id,
                                                                         unsigned long long* __restrict__ sums, int* __restrict__ members) {
  for (int64_t v = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    const int r = vert_rank[v];
    if (new_id[r] < 0) continue;  // no surviving triangle names the cell
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int q;
      dec_axis(pos[v * 3 + a], f.org[a], f.cel[a], f.n[a], &q);
      atomicAdd(sums + (size_t)r * 3 + a, (unsigned long long)q);
    }
    atomicAdd(members + r, 1);
  }
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_vertex_kernel(const DecFrame f, int n_ranks, int max_vertices,
                                                                            const int* __restrict__ new_id, const int* __restrict__ cell_of_rank,
                                                                            const unsigned long long* __restrict__ sums,
                                                                            const int* __restrict__ members, float* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; r < n_ranks; r += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    const int id = new_id[r];
    if (id < 0 || id >= max_vertices) continue;
    const int cell = cell_of_rank[r];
    const int idx[3] = {cell % f.n[0], (cell / f.n[0]) % f.n[1], cell / (f.n[0] * f.n[1])};
    const double n = (double)members[r];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double mean = ((double)sums[(size_t)r * 3 + a] / n) * 0x1p-20;  // one division, an exact scaling
      const double m = (double)f.org[a] + (double)f.cel[a] * ((double)idx[a] + mean);
      out[(size_t)id * 3 + a] = (float)m;
    }
  }
}

__global__ __launch_bounds__(RSN_DEC_BLOCK) void rsn_decimate_triangle_kernel(int T, int max_triangles, const int* __restrict__ tri,
                                                                              const int* __restrict__ tri_row, const int* __restrict__ vert_rank,
                                                                              const int* __restrict__ new_id, int* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * RSN_DEC_BLOCK + threadIdx.x; t < T; t += (int64_t)gridDim.x * RSN_DEC_BLOCK) {
    const int row = tri_row[t];
    if (row < 0 || row >= max_triangles) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(size_t)row * 3 + c] = new_id[vert_rank[tri[t * 3 + c]]];
  }
}

// ------------------------------------------------------------------------------------------------------------------- host side
static size_t dec_tiles(int64_t n) { return (size_t)((n + RSN_DEC_BLOCK - 1) / RSN_DEC_BLOCK); }
static unsigned dec_blocks(size_t tiles) { return (unsigned)(tiles < RSN_DEC_MAX_BLOCKS ? (tiles ? tiles : 1) : RSN_DEC_MAX_BLOCKS); }
static size_t dec_round8(size_t b) { return (b + 7) & ~(size_t)7; }

// Where everything lives in the workspace (byte offsets, every one a multiple of 8); R bounds the occupied cells.
struct DecLayout {
  int64_t cells, R;
  size_t sums, members, rank, cell_tiles, vert_rank, cell_of_rank, used, new_id, rank_tiles, keep, tri_row, tri_tiles, sign, total;
};

static bool dec_shape_ok(int32_t V, int32_t T, int32_t cx, int32_t cy, int32_t cz) {
  if (V < 0 || T < 0 || cx < 1 || cy < 1 || cz < 1) return false;
  const int64_t cxy = (int64_t)cx * cy;
  return cxy <= RSN_DEC_MAX_CELLS && cxy * cz <= RSN_DEC_MAX_CELLS;
}

static DecLayout dec_layout(int32_t V, int32_t T, int32_t cx, int32_t cy, int32_t cz) {
  DecLayout L;
  L.cells = (int64_t)cx * cy * cz;
  L.R = V < L.cells ? V : L.cells;
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t here = at;
    at += dec_round8(bytes);
    return here;
  };
  L.sums = take((size_t)L.R * 3 * sizeof(unsigned long long));
  L.members = take((size_t)L.R * sizeof(int));
  L.rank = take((size_t)L.cells * sizeof(int));
  L.cell_tiles = take((dec_tiles(L.cells) + 1) * sizeof(int));
  L.vert_rank = take((size_t)V * sizeof(int));
  L.cell_of_rank = take((size_t)L.R * sizeof(int));
  L.used = take((size_t)L.R * sizeof(int));
  L.new_id = take((size_t)L.R * sizeof(int));
  L.rank_tiles = take((dec_tiles(L.R) + 1) * sizeof(int));
  L.keep = take((size_t)T * sizeof(int));
  L.tri_row = take((size_t)T * sizeof(int));
  L.tri_tiles = take((dec_tiles(T) + 1) * sizeof(int));
  L.sign = take((size_t)T);
  L.total = at + 8;  // never 0
  return L;
}

extern "C" size_t rsn_decimate_workspace_bytes(int32_t n_vertices, int32_t n_triangles, int32_t cx, int32_t cy, int32_t cz) {
  if (!dec_shape_ok(n_vertices, n_triangles, cx, cy, cz)) {
    rsn_set_error("decimate: n_vertices=%d n_triangles=%d cells %d x %d x %d: need counts >= 0, every cell count >= 1 and at most 2^27 cells",
                  n_vertices, n_triangles, cx, cy, cz);
    return 0;
  }
  return dec_layout(n_vertices, n_triangles, cx, cy, cz).total;
}

// Everything the four calls check alike, in one order.
static int dec_prepare(const char* who, int32_t V, int32_t T, int32_t cx, int32_t cy, int32_t cz, const void* workspace,
                       size_t workspace_bytes, DecLayout* L) {
  RSN_REQUIRE(cx >= 1 && cy >= 1 && cz >= 1, RSN_ERR_INVALID_ARGUMENT, "%s: %d x %d x %d cells: every count must be at least 1", who, cx,
              cy, cz);
  RSN_REQUIRE(V >= 0 && T >= 0, RSN_ERR_INVALID_ARGUMENT, "%s: n_vertices=%d n_triangles=%d: need both >= 0", who, V, T);
  RSN_REQUIRE(dec_shape_ok(V, T, cx, cy, cz), RSN_ERR_UNSUPPORTED, "%s: %d x %d x %d cells: more than 2^27 (512^3)", who, cx, cy, cz);
  *L = dec_layout(V, T, cx, cy, cz);
  if (V == 0 || T == 0) return RSN_OK;  // nothing is launched: no workspace is needed
  RSN_REQUIRE(workspace, RSN_ERR_INVALID_ARGUMENT, "%s: workspace is NULL", who);
  RSN_REQUIRE(((uintptr_t)workspace & 7u) == 0, RSN_ERR_INVALID_ARGUMENT, "%s: workspace must be 8-byte aligned", who);
  RSN_REQUIRE(workspace_bytes >= L->total, RSN_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, L->total);
  return RSN_OK;
}

static int dec_frame(const char* who, int32_t cx, int32_t cy, int32_t cz, const float* origin3, const float* cell3, DecFrame* f) {
  RSN_REQUIRE(origin3 && cell3, RSN_ERR_INVALID_ARGUMENT, "%s: origin3 or cell3 is NULL", who);
  f->n[0] = cx; f->n[1] = cy; f->n[2] = cz;
  for (int a = 0; a < 3; ++a) {
    f->org[a] = origin3[a];
    f->cel[a] = cell3[a];
    RSN_REQUIRE(isfinite(f->org[a]) && isfinite(f->cel[a]) && f->cel[a] > 0.0f, RSN_ERR_INVALID_ARGUMENT,
                "%s: axis %d: origin %g cell size %g: need finite values and a cell size > 0", who, a, (double)f->org[a], (double)f->cel[a]);
  }
  return RSN_OK;
}

// flags src[0..n) -> dst (ranks or -1), the total -> *total, inverse as in the place kernel; tiles: (dec_tiles(n) + 1) ints
static void dec_compact(int64_t n, const int* src, int* dst, int* tiles, int* total, int* inverse, hipStream_t st) {
  const size_t n_tiles = dec_tiles(n);
  const dim3 grid(dec_blocks(n_tiles)), block(RSN_DEC_BLOCK);
  hipLaunchKernelGGL(rsn_decimate_tile_kernel, grid, block, 0, st, (int)n, (int)n_tiles, src, tiles);
  hipLaunchKernelGGL(rsn_decimate_scan_kernel, dim3(1), block, 0, st, (int)n_tiles, tiles, total);
  hipLaunchKernelGGL(rsn_decimate_place_kernel, grid, block, 0, st, (int)n, (int)n_tiles, src, dst, tiles, inverse);
}

extern "C" int rsn_decimate_cluster(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles,
                                    const float* origin3, const float* cell3, int32_t cx, int32_t cy, int32_t cz, void* workspace,
                                    size_t workspace_bytes, int64_t* keys, int32_t* counts, void* stream) {
  DecLayout L;
  DecFrame f;
  RSN_TRY(dec_prepare("decimate_cluster", n_vertices, n_triangles, cx, cy, cz, workspace, workspace_bytes, &L));
  RSN_TRY(dec_frame("decimate_cluster", cx, cy, cz, origin3, cell3, &f));
  RSN_REQUIRE(counts, RSN_ERR_INVALID_ARGUMENT, "decimate_cluster: counts is NULL");
  const bool empty = n_vertices == 0 || n_triangles == 0;
  RSN_REQUIRE(empty || (positions && triangles && keys), RSN_ERR_INVALID_ARGUMENT,
              "decimate_cluster: positions, triangles or keys is NULL");
  hipStream_t st = (hipStream_t)stream;
  RSN_HIP(hipMemsetAsync(counts, 0, 5 * sizeof(int32_t), st));
  if (empty) return RSN_OK;
  char* ws = (char*)workspace;
  int* rank = (int*)(ws + L.rank);
  int* vert = (int*)(ws + L.vert_rank);
  const dim3 block(RSN_DEC_BLOCK), vgrid(dec_blocks(dec_tiles(n_vertices))), tgrid(dec_blocks(dec_tiles(n_triangles)));
  RSN_HIP(hipMemsetAsync(rank, 0, (size_t)L.cells * sizeof(int), st));
  hipLaunchKernelGGL(rsn_decimate_cell_kernel, vgrid, block, 0, st, f, n_vertices, positions, vert, rank);
  dec_compact(L.cells, rank, rank, (int*)(ws + L.cell_tiles), counts + 4, (int*)(ws + L.cell_of_rank), st);
  hipLaunchKernelGGL(rsn_decimate_vert_rank_kernel, vgrid, block, 0, st, n_vertices, vert, rank);
  hipLaunchKernelGGL(rsn_decimate_key_kernel, tgrid, block, 0, st, n_vertices, n_triangles, triangles, vert, (long long*)keys,
                     (signed char*)(ws + L.sign), (int*)(ws + L.keep), counts);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_decimate_resolve(int32_t n_vertices, int32_t n_triangles, int32_t cx, int32_t cy, int32_t cz, const int64_t* sorted_keys,
                                    const int64_t* order, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
  DecLayout L;
  RSN_TRY(dec_prepare("decimate_resolve", n_vertices, n_triangles, cx, cy, cz, workspace, workspace_bytes, &L));
  if (n_vertices == 0 || n_triangles == 0) return RSN_OK;
  RSN_REQUIRE(sorted_keys && order && counts, RSN_ERR_INVALID_ARGUMENT, "decimate_resolve: sorted_keys, order or counts is NULL");
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(rsn_decimate_resolve_kernel, dim3(dec_blocks(dec_tiles(n_triangles))), dim3(RSN_DEC_BLOCK), 0, (hipStream_t)stream,
                     n_triangles, (const long long*)sorted_keys, (const long long*)order, (const signed char*)(ws + L.sign),
                     (int*)(ws + L.keep), counts);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_decimate_count(int32_t n_vertices, int32_t n_triangles, const int32_t* triangles, int32_t cx, int32_t cy, int32_t cz,
                                  void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
  DecLayout L;
  RSN_TRY(dec_prepare("decimate_count", n_vertices, n_triangles, cx, cy, cz, workspace, workspace_bytes, &L));
  if (n_vertices == 0 || n_triangles == 0) return RSN_OK;
  RSN_REQUIRE(triangles && counts, RSN_ERR_INVALID_ARGUMENT, "decimate_count: triangles or counts is NULL");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* used = (int*)(ws + L.used);
  int* keep = (int*)(ws + L.keep);
  RSN_HIP(hipMemsetAsync(used, 0, (size_t)L.R * sizeof(int), st));
  hipLaunchKernelGGL(rsn_decimate_used_kernel, dim3(dec_blocks(dec_tiles(n_triangles))), dim3(RSN_DEC_BLOCK), 0, st, n_triangles, triangles,
                     keep, (const int*)(ws + L.vert_rank), used);
  dec_compact(n_triangles, keep, (int*)(ws + L.tri_row), (int*)(ws + L.tri_tiles), counts + 1, nullptr, st);
  dec_compact(L.R, used, (int*)(ws + L.new_id), (int*)(ws + L.rank_tiles), counts, nullptr, st);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_decimate_emit(int32_t n_vertices, const float* positions, int32_t n_triangles, const int32_t* triangles,
                                 const float* origin3, const float* cell3, int32_t cx, int32_t cy, int32_t cz, void* workspace,
                                 size_t workspace_bytes, int32_t max_vertices, int32_t max_triangles, float* out_positions,
                                 int32_t* out_triangles, void* stream) {
  DecLayout L;
  DecFrame f;
  RSN_TRY(dec_prepare("decimate_emit", n_vertices, n_triangles, cx, cy, cz, workspace, workspace_bytes, &L));
  RSN_TRY(dec_frame("decimate_emit", cx, cy, cz, origin3, cell3, &f));
  RSN_REQUIRE(max_vertices >= 0 && max_triangles >= 0, RSN_ERR_INVALID_ARGUMENT,
              "decimate_emit: max_vertices=%d max_triangles=%d: need both >= 0", max_vertices, max_triangles);
  if (n_vertices == 0 || n_triangles == 0 || (max_vertices == 0 && max_triangles == 0)) return RSN_OK;
  RSN_REQUIRE(positions && triangles, RSN_ERR_INVALID_ARGUMENT, "decimate_emit: positions or triangles is NULL");
  RSN_REQUIRE((out_positions || max_vertices == 0) && (out_triangles || max_triangles == 0), RSN_ERR_INVALID_ARGUMENT,
              "decimate_emit: an output with a capacity above 0 is NULL");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int* vert = (const int*)(ws + L.vert_rank);
  const int* new_id = (const int*)(ws + L.new_id);
  const dim3 block(RSN_DEC_BLOCK);
  if (max_vertices > 0) {
    unsigned long long* sums = (unsigned long long*)(ws + L.sums);
    int* members = (int*)(ws + L.members);
    RSN_HIP(hipMemsetAsync(sums, 0, L.rank - L.sums, st));  // the sums and, behind them, the member counts
    hipLaunchKernelGGL(rsn_decimate_sum_kernel, dim3(dec_blocks(dec_tiles(n_vertices))), block, 0, st, f, n_vertices, positions, vert,
                       new_id, sums, members);
    hipLaunchKernelGGL(rsn_decimate_vertex_kernel, dim3(dec_blocks(dec_tiles(L.R))), block, 0, st, f, (int)L.R, max_vertices, new_id,
                       (const int*)(ws + L.cell_of_rank), sums, members, out_positions);
  }
  if (max_triangles > 0)
    hipLaunchKernelGGL(rsn_decimate_triangle_kernel, dim3(dec_blocks(dec_tiles(n_triangles))), block, 0, st, n_triangles, max_triangles,
                       triangles, (const int*)(ws + L.tri_row), vert, new_id, out_triangles);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
