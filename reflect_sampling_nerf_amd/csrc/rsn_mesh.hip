// Iso-surface extraction (include/rsn.h, "mesh export"): marching tetrahedra on the Kuhn split of every grid cell.
//
// No atomics, no hashing: every surface vertex lies on exactly one grid edge (v, dir), so its id is arithmetic on two
// scanned arrays, and every output slot is owned by one thread -- two runs give the same bits in the same order.
//
//   classify : one thread per grid vertex v.  Reads the 8 corners of the cell whose lowest corner is v and writes the
//              byte mask[v] = (inside(v) << 7) | crossing bits of the 7 edges v owns.  That byte alone also states the
//              inside / outside pattern of the whole cell (corner = inside(v) ^ crossing bit), hence its triangle count.
//              Per 1024-vertex block: the sums of both counts.
//   scan     : ONE 1024-thread workgroup turns the block sums into exclusive block bases, 1024 blocks per pass with a
//              carry (the second level of the scan), and publishes the two totals.
//   bases    : vbase[v] = block base + in-block exclusive scan of popcount(mask[v] & 0x7f); the id of edge (v, dir)
//              is vbase[v] + popcount(mask[v] & ((1 << dir) - 1)).
//   emit     : one thread per grid vertex: the positions of the edges it owns, and the triangles of its cell at the
//              block's triangle base + an in-block scan of the per-cell counts (recomputed from mask[v]).
//
// Workspace (rsn_mesh_workspace_bytes): [int32 vertex block bases: B][int32 triangle block bases: B][int32 vbase: N]
// [uint8 mask: N], B = ceil(N / 1024): 5 bytes per grid point + 8 per block.
#include "rsn_common.h"

#include <math.h>

#define RSN_MESH_BLOCK 1024                 // grid vertices per workgroup: the span of the first scan level
#define RSN_MESH_MAX_POINTS (1 << 27)       // 512^3: 8 v + dir and 12 triangles per cell fit an int32

// local corner L of a cell: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Direction number of the edge with offset L (nibble L):
// (1,0,0) 0, (0,1,0) 1, (0,0,1) 2, (1,1,0) 3, (1,0,1) 4, (0,1,1) 5, (1,1,1) 6
#define RSN_MESH_DIR_OF 0x65423100u
// tetrahedron p = 0..5 of a cell, one per axis permutation in lexicographic order xyz, xzy, yxz, yzx, zxy, zyx: its
// vertices are the corners 0, L1[p], L2[p], 7 (nibble p); the odd permutations (p = 1, 2, 5) are negatively oriented
#define RSN_MESH_L1 0x442211u
#define RSN_MESH_L2 0x656353u
#define RSN_MESH_NEG 0x26u

struct MeshWs {
  int32_t* vblock;
  int32_t* tblock;
  int32_t* vbase;
  uint8_t* mask;
};

static MeshWs mesh_ws(void* workspace, int64_t n) {
  const int64_t nblk = (n + RSN_MESH_BLOCK - 1) / RSN_MESH_BLOCK;
  int32_t* w = (int32_t*)workspace;
  return MeshWs{w, w + nblk, w + 2 * nblk, (uint8_t*)(w + 2 * nblk + n)};
}

// inside / outside of the 8 corners of the cell at v (bit L) from its mask byte
__device__ __forceinline__ unsigned mesh_corners(unsigned mb) {
  const unsigned in0 = mb >> 7;
  unsigned cb = in0;
#pragma unroll
  for (int L = 1; L < 8; ++L) cb |= (in0 ^ ((mb >> ((RSN_MESH_DIR_OF >> (4 * L)) & 15u)) & 1u)) << L;
  return cb;
}

// nibble q = corner of tetrahedron p's vertex q
__device__ __forceinline__ unsigned mesh_tet(int p) {
  return (((RSN_MESH_L1 >> (4 * p)) & 15u) << 4) | (((RSN_MESH_L2 >> (4 * p)) & 15u) << 8) | (7u << 12);
}

// the 4 inside bits of tetrahedron `tet` (mesh_tet) in a cell with corner bits cb
__device__ __forceinline__ unsigned mesh_tet_inside(unsigned tet, unsigned cb) {
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) m |= ((cb >> ((tet >> (4 * q)) & 15u)) & 1u) << q;
  return m;
}

__device__ __forceinline__ int mesh_cell_triangles(unsigned cb) {
  int t = 0;
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const int n = __builtin_popcount(mesh_tet_inside(mesh_tet(p), cb));
    t += (n == 0 || n == 4) ? 0 : (n == 2 ? 2 : 1);
  }
  return t;
}

// exclusive scan of x over the 1024-thread workgroup; *total = the workgroup's sum.  s_wave: 16 ints of LDS.
__device__ __forceinline__ int mesh_block_scan(int x, int* s_wave, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int incl = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(incl, off, 64);
    if (lane >= off) incl += y;
  }
  __syncthreads();  // the previous use of s_wave is over
  if (lane == 63) s_wave[wid] = incl;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const int t = s_wave[w];
    if (w < wid) before += t;
    tot += t;
  }
  *total = tot;
  return before + incl - x;
}

__global__ __launch_bounds__(RSN_MESH_BLOCK) void rsn_mesh_classify_kernel(int nx, int ny, int nz, const float* __restrict__ vol,
                                                                           float iso, MeshWs ws) {
  __shared__ int s_wave[16];
  const int n = nx * ny * nz;
  const int v = blockIdx.x * RSN_MESH_BLOCK + threadIdx.x;
  int nv = 0, nt = 0;
  if (v < n) {
    const int i = v % nx, j = (v / nx) % ny, k = v / (nx * ny);
    const bool ex = i + 1 < nx, ey = j + 1 < ny, ez = k + 1 < nz;
    const unsigned in0 = vol[v] >= iso ? 1u : 0u;  // NaN: outside
    unsigned mb = in0 << 7;
#pragma unroll
    for (int L = 1; L < 8; ++L) {
      const bool exists = (!(L & 1) || ex) && (!(L & 2) || ey) && (!(L & 4) || ez);
      if (exists) {
        const int vf = v + (L & 1) + ((L >> 1) & 1) * nx + ((L >> 2) & 1) * nx * ny;
        const unsigned inf_ = vol[vf] >= iso ? 1u : 0u;
        mb |= (inf_ ^ in0) << ((RSN_MESH_DIR_OF >> (4 * L)) & 15u);
      }
    }
    ws.mask[v] = (uint8_t)mb;
    nv = __builtin_popcount(mb & 0x7fu);
    if (ex && ey && ez) nt = mesh_cell_triangles(mesh_corners(mb));
  }
  int tv, tt;
  mesh_block_scan(nv, s_wave, &tv);
  mesh_block_scan(nt, s_wave, &tt);
  if (threadIdx.x == 0) {
    ws.vblock[blockIdx.x] = tv;
    ws.tblock[blockIdx.x] = tt;
  }
}

// second scan level: block sums -> exclusive block bases, RSN_MESH_BLOCK of them per pass; counts[] = the totals
__global__ __launch_bounds__(RSN_MESH_BLOCK) void rsn_mesh_scan_kernel(int nblk, MeshWs ws, int32_t* counts) {
  __shared__ int s_wave[16];
  int carry_v = 0, carry_t = 0;
  for (int base = 0; base < nblk; base += RSN_MESH_BLOCK) {
    const int b = base + threadIdx.x;
    const int xv = b < nblk ? ws.vblock[b] : 0, xt = b < nblk ? ws.tblock[b] : 0;
    int tv, tt;
    const int ev = mesh_block_scan(xv, s_wave, &tv);
    const int et = mesh_block_scan(xt, s_wave, &tt);
    if (b < nblk) {
      ws.vblock[b] = carry_v + ev;
      ws.tblock[b] = carry_t + et;
    }
    carry_v += tv;
    carry_t += tt;
  }
  if (threadIdx.x == 0) {
    counts[0] = carry_v;
    counts[1] = carry_t;
  }
}

__global__ __launch_bounds__(RSN_MESH_BLOCK) void rsn_mesh_bases_kernel(int n, MeshWs ws) {
  __shared__ int s_wave[16];
  const int v = blockIdx.x * RSN_MESH_BLOCK + threadIdx.x;
  const int nv = v < n ? __builtin_popcount(ws.mask[v] & 0x7fu) : 0;
  int tot;
  const int e = mesh_block_scan(nv, s_wave, &tot);
  if (v < n) ws.vbase[v] = ws.vblock[blockIdx.x] + e;
}

struct MeshFrame {
  float o[3], s[3];
};

// id of the surface vertex on the edge between vertices qa and qb of tetrahedron `tet` in the cell at v
__device__ __forceinline__ int mesh_edge_id(const MeshWs& ws, int v, int nx, int nxy, unsigned tet, int qa, int qb) {
  const int lo = qa < qb ? qa : qb, hi = qa < qb ? qb : qa;
  const unsigned Llo = (tet >> (4 * lo)) & 15u, Lhi = (tet >> (4 * hi)) & 15u;
  const unsigned dir = (RSN_MESH_DIR_OF >> (4 * (Llo ^ Lhi))) & 15u;
  const int owner = v + (int)(Llo & 1u) + (int)((Llo >> 1) & 1u) * nx + (int)((Llo >> 2) & 1u) * nxy;
  return ws.vbase[owner] + __builtin_popcount(ws.mask[owner] & ((1u << dir) - 1u));
}

__device__ __forceinline__ void mesh_put_triangle(int32_t* triangles, int t, int max_triangles, int a, int b, int c, bool flip) {
  if (t < max_triangles) {
    int32_t* o = triangles + (size_t)t * 3;
    o[0] = a;
    o[1] = flip ? c : b;
    o[2] = flip ? b : c;
  }
}

__global__ __launch_bounds__(RSN_MESH_BLOCK) void rsn_mesh_emit_kernel(int nx, int ny, int nz, const float* __restrict__ vol,
                                                                       float iso, MeshFrame fr, MeshWs ws, int max_vertices,
                                                                       int max_triangles, float* __restrict__ positions,
                                                                       int32_t* __restrict__ vert_key,
                                                                       int32_t* __restrict__ triangles) {
  __shared__ int s_wave[16];
  const int n = nx * ny * nz, nxy = nx * ny;
  const int v = blockIdx.x * RSN_MESH_BLOCK + threadIdx.x;
  unsigned mb = 0;
  int nt = 0;
  bool cell = false;
  int i = 0, j = 0, k = 0;
  if (v < n) {
    i = v % nx, j = (v / nx) % ny, k = v / nxy;
    mb = ws.mask[v];
    cell = i + 1 < nx && j + 1 < ny && k + 1 < nz;
  }
  const unsigned cb = mesh_corners(mb);
  if (cell) nt = mesh_cell_triangles(cb);
  int tot;
  int t_out = ws.tblock[blockIdx.x] + mesh_block_scan(nt, s_wave, &tot);

  // ---- the surface vertices on the edges this grid vertex owns, ascending dir
  int id = (mb & 0x7fu) ? ws.vbase[v] : 0;
  if ((mb & 0x7fu) && id < max_vertices) {
    const float f_lo = vol[v];
    const float plo[3] = {fr.o[0] + fr.s[0] * (float)i, fr.o[1] + fr.s[1] * (float)j, fr.o[2] + fr.s[2] * (float)k};
#pragma unroll
    for (int dir = 0; dir < 7; ++dir) {
      if (!((mb >> dir) & 1u)) continue;
      if (id >= max_vertices) break;
      // offset of direction dir: 0..2 the axes, 3 = xy, 4 = xz, 5 = yz, 6 = xyz
      const int L = dir < 3 ? (1 << dir) : (dir == 3 ? 3 : (dir == 4 ? 5 : (dir == 5 ? 6 : 7)));
      const int d[3] = {L & 1, (L >> 1) & 1, (L >> 2) & 1};
      const float f_hi = vol[v + d[0] + d[1] * nx + d[2] * nxy];
      float t = (iso - f_lo) / (f_hi - f_lo);
      t = (t != t) ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
      const int c3[3] = {i, j, k};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float phi = fr.o[c] + fr.s[c] * (float)(c3[c] + d[c]);
        const float p = plo[c] + t * (phi - plo[c]);
        positions[(size_t)id * 3 + c] = fminf(fmaxf(p, plo[c]), phi);  // on the edge whatever the rounding did
      }
      if (vert_key) vert_key[id] = v * 8 + dir;
      ++id;
    }
  }

  // ---- the triangles of the cell at v: tetrahedra in permutation order
  if (nt == 0 || t_out >= max_triangles) return;
#pragma unroll 1
  for (int p = 0; p < 6; ++p) {
    const unsigned tet = mesh_tet(p);
    const unsigned m = mesh_tet_inside(tet, cb);
    const int cnt = __builtin_popcount(m);
    if (cnt == 0 || cnt == 4) continue;
    const bool neg = (RSN_MESH_NEG >> p) & 1u;
    if (cnt != 2) {
      // one vertex on its own side: the triangle on its three edges; (lone, others ascending) is an even permutation of
      // (0,1,2,3) when lone is even, and then, in a positive tetrahedron with lone inside, the normal points away from it
      const int lone = __builtin_ctz(cnt == 1 ? m : (~m & 15u));
      const int o[3] = {lone == 0 ? 1 : 0, lone <= 1 ? 2 : 1, lone <= 2 ? 3 : 2};  // the others, ascending
      const bool flip = ((lone & 1) != 0) ^ (cnt == 3) ^ neg;
      mesh_put_triangle(triangles, t_out++, max_triangles, mesh_edge_id(ws, v, nx, nxy, tet, lone, o[0]),
                        mesh_edge_id(ws, v, nx, nxy, tet, lone, o[1]), mesh_edge_id(ws, v, nx, nxy, tet, lone, o[2]), flip);
    } else {
      // inside a < b, outside c < d: the quad ac, ad, bd, bc as (ac, ad, bd), (ac, bd, bc); (a,b,c,d) has a + b - 1 inversions
      const unsigned out = ~m & 15u;
      const int a = __builtin_ctz(m), b = 31 - __builtin_clz(m), c = __builtin_ctz(out), d = 31 - __builtin_clz(out);
      const bool flip = (((a + b) & 1) == 0) ^ neg;
      const int ac = mesh_edge_id(ws, v, nx, nxy, tet, a, c), ad = mesh_edge_id(ws, v, nx, nxy, tet, a, d);
      const int bd = mesh_edge_id(ws, v, nx, nxy, tet, b, d), bc = mesh_edge_id(ws, v, nx, nxy, tet, b, c);
      mesh_put_triangle(triangles, t_out++, max_triangles, ac, ad, bd, flip);
      mesh_put_triangle(triangles, t_out++, max_triangles, ac, bd, bc, flip);
    }
  }
}

static int mesh_check_dims(int32_t nx, int32_t ny, int32_t nz) {
  RSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, RSN_ERR_INVALID_ARGUMENT,
              "mesh grid %d x %d x %d: every dimension must be at least 2", nx, ny, nz);
  const int64_t nxy = (int64_t)nx * ny;
  RSN_REQUIRE(nxy <= RSN_MESH_MAX_POINTS && nxy * nz <= RSN_MESH_MAX_POINTS, RSN_ERR_UNSUPPORTED,
              "mesh grid %d x %d x %d: more than 2^27 points (512^3)", nx, ny, nz);
  return RSN_OK;
}

extern "C" size_t rsn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (mesh_check_dims(nx, ny, nz) != RSN_OK) return 0;
  const int64_t n = (int64_t)nx * ny * nz, nblk = (n + RSN_MESH_BLOCK - 1) / RSN_MESH_BLOCK;
  return (size_t)((8 * nblk + 5 * n + 15) / 16 * 16);
}

extern "C" int rsn_mesh_count(int32_t nx, int32_t ny, int32_t nz, const float* vol, float iso, void* workspace,
                              size_t workspace_bytes, int32_t* counts, void* stream) {
  RSN_TRY(mesh_check_dims(nx, ny, nz));
  RSN_REQUIRE(vol && workspace && counts, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  const size_t need = rsn_mesh_workspace_bytes(nx, ny, nz);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  RSN_REQUIRE(((uintptr_t)workspace & 3) == 0, RSN_ERR_INVALID_ARGUMENT, "workspace must be 4-byte aligned");
  const int n = nx * ny * nz, nblk = (n + RSN_MESH_BLOCK - 1) / RSN_MESH_BLOCK;
  const MeshWs ws = mesh_ws(workspace, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rsn_mesh_classify_kernel, dim3(nblk), dim3(RSN_MESH_BLOCK), 0, st, nx, ny, nz, vol, iso, ws);
  hipLaunchKernelGGL(rsn_mesh_scan_kernel, dim3(1), dim3(RSN_MESH_BLOCK), 0, st, nblk, ws, counts);
  hipLaunchKernelGGL(rsn_mesh_bases_kernel, dim3(nblk), dim3(RSN_MESH_BLOCK), 0, st, n, ws);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}

extern "C" int rsn_mesh_emit(int32_t nx, int32_t ny, int32_t nz, const float* vol, float iso, const float* origin3,
                             const float* spacing3, const void* workspace, size_t workspace_bytes, int32_t max_vertices,
                             int32_t max_triangles, float* positions, int32_t* vert_key, int32_t* triangles, void* stream) {
  RSN_TRY(mesh_check_dims(nx, ny, nz));
  RSN_REQUIRE(vol && workspace && origin3 && spacing3, RSN_ERR_INVALID_ARGUMENT, "a pointer is NULL");
  RSN_REQUIRE(max_vertices >= 0 && max_triangles >= 0, RSN_ERR_INVALID_ARGUMENT, "max_vertices=%d max_triangles=%d",
              max_vertices, max_triangles);
  RSN_REQUIRE((max_vertices == 0 || positions) && (max_triangles == 0 || triangles), RSN_ERR_INVALID_ARGUMENT,
              "an output pointer is NULL");
  const size_t need = rsn_mesh_workspace_bytes(nx, ny, nz);
  RSN_REQUIRE(workspace_bytes >= need, RSN_ERR_WORKSPACE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  RSN_REQUIRE(((uintptr_t)workspace & 3) == 0, RSN_ERR_INVALID_ARGUMENT, "workspace must be 4-byte aligned");
  MeshFrame fr;
  const int dims[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) {
    fr.o[c] = origin3[c];
    fr.s[c] = spacing3[c];
    // the far corner in the kernel's own arithmetic: finite, so that every position is
    RSN_REQUIRE(isfinite(fr.o[c]) && fr.s[c] > 0.0f && isfinite(fr.o[c] + fr.s[c] * (float)(dims[c] - 1)),
                RSN_ERR_INVALID_ARGUMENT, "origin[%d]=%g spacing[%d]=%g: need a finite box and a positive spacing", c,
                (double)fr.o[c], c, (double)fr.s[c]);
  }
  if (max_vertices == 0 && max_triangles == 0) return RSN_OK;
  const int n = nx * ny * nz, nblk = (n + RSN_MESH_BLOCK - 1) / RSN_MESH_BLOCK;
  const MeshWs ws = mesh_ws(const_cast<void*>(workspace), n);
  hipLaunchKernelGGL(rsn_mesh_emit_kernel, dim3(nblk), dim3(RSN_MESH_BLOCK), 0, (hipStream_t)stream, nx, ny, nz, vol, iso, fr,
                     ws, max_vertices, max_triangles, positions, vert_key, triangles);
  RSN_HIP(hipGetLastError());
  return RSN_OK;
}
