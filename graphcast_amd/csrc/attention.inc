// attention.inc -- GenCast's mesh transformer (weathernext1_gen/transformer.py, utils/sparse_transformer.py) on
// gfx950: the k-hop block-sparse attention and the small row kernels around it.  Included at the end of gcast.hip
// (it reuses mfma16 / mfma32h / split2 / split8 / check_launch / fail from there).
//
// Attention (sparse_transformer.py mha / triblockdiag_mha / splash_mha: all three compute the same function)
//   out[b, t, 128 h : 128 h + 128] = sum_T softmax_T(q_t . k_T / sqrt(128) | mask[t, T]) v_T
// over the nodes of an internal order (graphcast_amd/sparse_transformer.py picks it), cut into 64-row tiles.  A
// work unit is one (query tile, head, batch element): one workgroup of four waves, 16 query rows per wave.  It walks
// the CSR list of the key tiles its mask touches; every (query tile, key tile) pair carries 64 words of 64 bits --
// bit c of word r: query row r may attend key row c of the key tile.  Per key tile:
//   S^T = K . Q^T     (A = K rows from LDS, B = Q held in registers: lane l = 16 g + n owns query row n, and the
//                      accumulator of key block nb holds S^T[16 nb + 4 g + r][n] -- the 16 scores a lane owns all
//                      belong to ONE query row, so the row maximum / sum need two lane swaps only)
//   online softmax in fp32 (running max m and sum l per query row; masked keys contribute exactly 0)
//   O^T += V^T . P^T  (A = V from LDS, B = P straight from the score registers)
// and the workgroup stores O / l, head-concatenated, as [rows, 512].  Every sum has a fixed order: no atomics, no
// cross-workgroup reduction -- bitwise repeatable.
//
// Arithmetic, as in the row-MLP kernels (include/gcast.h, gc_precision):
//   GC_PREC_F32    v_mfma_f32_16x16x4_f32 for both products: exact fp32 products;
//   GC_PREC_F16X3  every operand split into fp16 halves (hi, lo) and each product formed as hi.hi + lo.hi + hi.lo
//                  by three v_mfma_f32_16x16x32_f16 (K^T and V^T are split once when a tile is staged, Q once per
//                  work unit, P once per key tile, pre-scaled by 2^10 so that its lo halves stay normal numbers).
//                  A Q, K or V value beyond GC_F16X3_MAX sets *range_flag (the contract of gc_rowmlp_desc.range_flag).
namespace {

constexpr int kAtTile = GC_ATTN_TILE;      // 64 query rows / key rows per tile
constexpr int kAtHead = GC_ATTN_HEAD;      // 128 = key size = value size
constexpr int kAtKs = kAtHead + 4;         // f32: padded LDS row of K / V (floats): conflict-free fragment reads
constexpr int kAtKh = kAtHead + 8;         // f16x3: padded LDS row of the K halves (halves)
constexpr int kAtVt = kAtTile + 8;         // f16x3: padded LDS row of the TRANSPOSED V halves (halves)
constexpr float kAtPScale = 1024.f;        // f16x3: P is split as P * 2^10 (lo halves normal down to p ~ 1e-7)
constexpr float kAtMaskFill = -1e30f;      // the reference's fill value (sparse_transformer.py mha)

__device__ __forceinline__ bool at_out_of_range(f4 v) {
  return fabsf(v.x) > GC_F16X3_MAX || fabsf(v.y) > GC_F16X3_MAX || fabsf(v.z) > GC_F16X3_MAX ||
         fabsf(v.w) > GC_F16X3_MAX;
}

__device__ __forceinline__ f4 at_load_row4(const float* __restrict__ base, int row, int n_rows, long ld, int col) {
  if (row >= n_rows) return f4{0.f, 0.f, 0.f, 0.f};
  return *reinterpret_cast<const f4*>(base + (long)row * ld + col);
}

// F16X3 = 0: LDS = K [64][132] floats | V [64][132] floats                      (67.6 KiB)
// F16X3 = 1: LDS = K hi, K lo [64][136] halves | V^T hi, V^T lo [128][72] halves (71.8 KiB)
template <int F16X3>
__global__ __launch_bounds__(256, 2) void attn_tile_kernel(
    int n_rows, const int* __restrict__ tile_ptr, const int* __restrict__ tile_col,
    const unsigned long long* __restrict__ tile_bits, const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, int ld, float scale, float* __restrict__ out, int ldo, int* __restrict__ range_flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char at_lds[];
  const int qt = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const long boff = (long)b * n_rows * ld;
  const float* qb = q + boff;
  const float* kb = k + boff;
  const float* vb = v + boff;
  const int hcol = head * kAtHead;
  const int qrow = qt * kAtTile + 16 * wave + n;          // the query row this lane owns
  bool bad = false;

  // ---- Q fragment (B operand of S^T = K . Q^T), once per work unit
  float qf[32];                   // F16X3 = 0: qf[s] = Q[qrow][32 g + s]
  u4 qh[4], ql[4];                // F16X3 = 1: K step s: Q[qrow][32 s + 8 g + j], split
  if constexpr (!F16X3) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f4 x = at_load_row4(qb, qrow, n_rows, ld, hcol + 32 * g + 4 * c);
      qf[4 * c] = x.x; qf[4 * c + 1] = x.y; qf[4 * c + 2] = x.z; qf[4 * c + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f4 x0 = at_load_row4(qb, qrow, n_rows, ld, hcol + 32 * s + 8 * g);
      const f4 x1 = at_load_row4(qb, qrow, n_rows, ld, hcol + 32 * s + 8 * g + 4);
      bad |= at_out_of_range(x0) | at_out_of_range(x1);
      split8(x0, x1, qh[s], ql[s]);
    }
  }

  f4 o[8];                        // O^T[16 db + 4 g + r][query n]
#pragma unroll
  for (int db = 0; db < 8; ++db) o[db] = f4{0.f, 0.f, 0.f, 0.f};
  float m = kAtMaskFill, l = 0.f; // running max (every lane of a row holds it) / this lane's share of the sum

  const int t0 = tile_ptr[qt], t1 = tile_ptr[qt + 1];
  for (int t = t0; t < t1; ++t) {
    const int kt = tile_col[t];
    const int krow0 = kt * kAtTile;
    __syncthreads();              // every wave is done with the previous tile's K / V
    // ---- stage K and V of key tile kt (rows past n_rows are zeros; the mask never selects them)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int f = tid + 256 * it;                     // float4 index in the 64 x 128 tile
      const int row = f >> 5, c4 = (f & 31) * 4;
      const f4 kx = at_load_row4(kb, krow0 + row, n_rows, ld, hcol + c4);
      const f4 vx = at_load_row4(vb, krow0 + row, n_rows, ld, hcol + c4);
      if constexpr (!F16X3) {
        float* ks = reinterpret_cast<float*>(at_lds);
        float* vs = ks + kAtTile * kAtKs;
        *reinterpret_cast<f4*>(ks + row * kAtKs + c4) = kx;
        *reinterpret_cast<f4*>(vs + row * kAtKs + c4) = vx;
      } else {
        bad |= at_out_of_range(kx) | at_out_of_range(vx);
        unsigned short* kh = reinterpret_cast<unsigned short*>(at_lds);
        unsigned short* kl = kh + kAtTile * kAtKh;
        unsigned short* vth = kl + kAtTile * kAtKh;
        unsigned short* vtl = vth + kAtHead * kAtVt;
        unsigned h0, h1, l0, l1;
        split2(kx.x, kx.y, h0, l0);
        split2(kx.z, kx.w, h1, l1);
        *reinterpret_cast<uint2*>(kh + row * kAtKh + c4) = uint2{h0, h1};
        *reinterpret_cast<uint2*>(kl + row * kAtKh + c4) = uint2{l0, l1};
        split2(vx.x, vx.y, h0, l0);
        split2(vx.z, vx.w, h1, l1);
        vth[(c4 + 0) * kAtVt + row] = (unsigned short)(h0 & 0xffffu);
        vth[(c4 + 1) * kAtVt + row] = (unsigned short)(h0 >> 16);
        vth[(c4 + 2) * kAtVt + row] = (unsigned short)(h1 & 0xffffu);
        vth[(c4 + 3) * kAtVt + row] = (unsigned short)(h1 >> 16);
        vtl[(c4 + 0) * kAtVt + row] = (unsigned short)(l0 & 0xffffu);
        vtl[(c4 + 1) * kAtVt + row] = (unsigned short)(l0 >> 16);
        vtl[(c4 + 2) * kAtVt + row] = (unsigned short)(l1 & 0xffffu);
        vtl[(c4 + 3) * kAtVt + row] = (unsigned short)(l1 >> 16);
      }
    }
    const unsigned long long bits = tile_bits[(long)t * kAtTile + 16 * wave + n];
    __syncthreads();

    // ---- S^T = K . Q^T: sc[nb][r] = S[query n][key 16 nb + 4 g + r]
    f4 sc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) sc[nb] = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (!F16X3) {
      const float* ks = reinterpret_cast<const float*>(at_lds);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const float* kr = ks + (16 * nb + n) * kAtKs + 32 * g;   // A[i = n][k = g] = K[16 nb + i][32 g + s]
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const f4 a = *reinterpret_cast<const f4*>(kr + 4 * c);
          sc[nb] = mfma16(a.x, qf[4 * c + 0], sc[nb]);
          sc[nb] = mfma16(a.y, qf[4 * c + 1], sc[nb]);
          sc[nb] = mfma16(a.z, qf[4 * c + 2], sc[nb]);
          sc[nb] = mfma16(a.w, qf[4 * c + 3], sc[nb]);
        }
      }
    } else {
      const unsigned short* kh = reinterpret_cast<const unsigned short*>(at_lds);
      const unsigned short* kl = kh + kAtTile * kAtKh;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int off = (16 * nb + n) * kAtKh + 32 * s + 8 * g;   // A[i][8 g + j] = K[16 nb + i][32 s + 8 g + j]
          const u4 ah = *reinterpret_cast<const u4*>(kh + off);
          const u4 al = *reinterpret_cast<const u4*>(kl + off);
          sc[nb] = mfma32h(al, qh[s], sc[nb]);
          sc[nb] = mfma32h(ah, ql[s], sc[nb]);
          sc[nb] = mfma32h(ah, qh[s], sc[nb]);
        }
      }
    }

    // ---- online softmax (fp32)
    float mt = kAtMaskFill;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = (bits >> (16 * nb + 4 * g + r)) & 1ull;
        const float s = on ? sc[nb][r] * scale : kAtMaskFill;
        sc[nb][r] = s;
        mt = fmaxf(mt, s);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m, mt);
    const float alpha = expf(m - m_new);
    float psum = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = (bits >> (16 * nb + 4 * g + r)) & 1ull;
        const float p = on ? expf(sc[nb][r] - m_new) : 0.f;
        sc[nb][r] = p;
        psum += p;
      }
    }
    l = l * alpha + psum;
    m = m_new;
#pragma unroll
    for (int db = 0; db < 8; ++db) o[db] *= alpha;

    // ---- O^T += V^T . P^T
    if constexpr (!F16X3) {
      const float* vs = reinterpret_cast<const float*>(at_lds) + kAtTile * kAtKs;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // K step (nb, r): k index g <-> key 16 nb + 4 g + r; A[i][g] = V[key][16 db + i], B[g][n] = this lane's p
          const float* vr = vs + (16 * nb + 4 * g + r) * kAtKs + n;
#pragma unroll
          for (int db = 0; db < 8; ++db) o[db] = mfma16(vr[16 * db], sc[nb][r], o[db]);
        }
      }
    } else {
      const unsigned short* vth = reinterpret_cast<const unsigned short*>(at_lds) + 2 * kAtTile * kAtKh;
      const unsigned short* vtl = vth + kAtHead * kAtVt;
#pragma unroll
      for (int ts = 0; ts < 2; ++ts) {
        // K step ts covers key blocks 2 ts, 2 ts + 1: element j of lane group g is key 32 ts + 4 g + j (j < 4) and
        // 32 ts + 16 + 4 g + j - 4 (j >= 4) -- the registers of those two score blocks as they are (gcast.h "chained")
        u4 ph, pl;
        split8(sc[2 * ts] * kAtPScale, sc[2 * ts + 1] * kAtPScale, ph, pl);
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          const int off = (16 * db + n) * kAtVt + 32 * ts + 4 * g;
          const uint2 h0 = *reinterpret_cast<const uint2*>(vth + off);
          const uint2 h1 = *reinterpret_cast<const uint2*>(vth + off + 16);
          const uint2 l0 = *reinterpret_cast<const uint2*>(vtl + off);
          const uint2 l1 = *reinterpret_cast<const uint2*>(vtl + off + 16);
          const u4 ah = u4{h0.x, h0.y, h1.x, h1.y}, al = u4{l0.x, l0.y, l1.x, l1.y};
          o[db] = mfma32h(al, ph, o[db]);
          o[db] = mfma32h(ah, pl, o[db]);
          o[db] = mfma32h(ah, ph, o[db]);
        }
      }
    }
  }

  if constexpr (F16X3) {
    if (bad && range_flag) *range_flag = 1;
  }
  // ---- normalised store: out[qrow][128 head + 16 db + 4 g + r]
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qrow < n_rows) {
    const float inv = (F16X3 ? 1.f / kAtPScale : 1.f) / l;
    float* orow = out + (long)b * n_rows * ldo + (long)qrow * ldo + hcol + 4 * g;
#pragma unroll
    for (int db = 0; db < 8; ++db) *reinterpret_cast<f4*>(orow + 16 * db) = o[db] * inv;
  }
}

// out[r] = LayerNorm(x[r]) * scale[b] + offset[b], b = r / rows_per_batch: haiku LayerNorm without its own scale /
// offset (eps 1e-5, biased variance) followed by dense.LinearNormConditioning's (1 + s_b, o_b) (the + 1 is folded
// into `scale` by the host).  One wave per 512-wide row.
__global__ __launch_bounds__(256) void ln_cond_kernel(int n_rows, int rows_per_batch, const float* __restrict__ x,
                                                      const float* __restrict__ scale,
                                                      const float* __restrict__ offset, float* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  const float* xr = x + (long)row * kD;
  const f4 a = *reinterpret_cast<const f4*>(xr + 4 * lane);
  const f4 c = *reinterpret_cast<const f4*>(xr + 256 + 4 * lane);
  float s = (a.x + a.y) + (a.z + a.w) + (c.x + c.y) + (c.z + c.w);
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w);
  const float mean = s * (1.f / kD);
  const f4 da = a - mean, dc = c - mean;
  float q = (da.x * da.x + da.y * da.y) + (da.z * da.z + da.w * da.w) + (dc.x * dc.x + dc.y * dc.y) +
            (dc.z * dc.z + dc.w * dc.w);
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) q += __shfl_xor(q, w);
  const float rs = 1.f / sqrtf(q * (1.f / kD) + kLnEps);
  const int b = row / rows_per_batch;
  const float* sb = scale + (long)b * kD;
  const float* ob = offset + (long)b * kD;
  const f4 s0 = *reinterpret_cast<const f4*>(sb + 4 * lane), s1 = *reinterpret_cast<const f4*>(sb + 256 + 4 * lane);
  const f4 o0 = *reinterpret_cast<const f4*>(ob + 4 * lane), o1 = *reinterpret_cast<const f4*>(ob + 256 + 4 * lane);
  float* orow = out + (long)row * kD;
  *reinterpret_cast<f4*>(orow + 4 * lane) = da * rs * s0 + o0;
  *reinterpret_cast<f4*>(orow + 256 + 4 * lane) = dc * rs * s1 + o1;
}

// x <- jax.nn.gelu(x) (approximate=True, jax's default): 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))).
__global__ __launch_bounds__(256) void gelu_kernel(long n4, float* __restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f4 v = reinterpret_cast<f4*>(x)[i];
  const float c = 0.7978845608028654f;     // sqrt(2 / pi)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = v[e];
    v[e] = 0.5f * y * (1.f + tanhf(c * (y + 0.044715f * y * y * y)));
  }
  reinterpret_cast<f4*>(x)[i] = v;
}

// dst[r] = src[idx[r]] for 512-wide rows, independently per batch element: the node order of the caller <-> the
// internal order of the tiles.  src / dst [batch, rows, 512] with batch strides src_bstride / dst_bstride (rows)
// and row strides ld_src / ld_dst (floats).
__global__ __launch_bounds__(128) void permute_rows_kernel(int n, const int* __restrict__ idx,
                                                           const float* __restrict__ src, long src_bstride,
                                                           int ld_src, float* __restrict__ dst, long dst_bstride,
                                                           int ld_dst) {
  const int r = blockIdx.x, b = blockIdx.y;
  const f4 x = *reinterpret_cast<const f4*>(src + b * src_bstride * ld_src + (long)idx[r] * ld_src + 4 * threadIdx.x);
  *reinterpret_cast<f4*>(dst + b * dst_bstride * ld_dst + (long)r * ld_dst + 4 * threadIdx.x) = x;
}

bool g_attn_attr_set[2] = {false, false};

}  // namespace

extern "C" {

int gc_attention(int prec, int batch, int n_rows, int n_qtiles, const int* tile_ptr, const int* tile_col,
                 const unsigned long long* tile_bits, const float* q, const float* k, const float* v, int ld,
                 float scale, float* out, int ldo, int* range_flag, void* stream) {
  if (prec != GC_PREC_F32 && prec != GC_PREC_F16X3) return fail(GC_EINVAL, "gc_attention: prec must be f32 or f16x3");
  if (batch <= 0 || n_rows <= 0 || n_qtiles != (n_rows + kAtTile - 1) / kAtTile || batch > 65535)
    return fail(GC_EINVAL, "gc_attention: bad sizes (n_qtiles must be ceil(n_rows / 64))");
  if (!tile_ptr || !tile_col || !tile_bits || !q || !k || !v || !out)
    return fail(GC_EINVAL, "gc_attention: null pointer");
  if ((ld & 3) || (ldo & 3) || ld < GC_ATTN_HEADS * kAtHead || ldo < GC_ATTN_HEADS * kAtHead ||
      ((reinterpret_cast<size_t>(q) | reinterpret_cast<size_t>(k) | reinterpret_cast<size_t>(v) |
        reinterpret_cast<size_t>(out)) & 15))
    return fail(GC_EINVAL, "gc_attention: rows must be 16-byte aligned with strides >= 512 (multiples of 4)");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(n_qtiles, GC_ATTN_HEADS, batch);
  if (prec == GC_PREC_F32) {
    const size_t lds = 2 * kAtTile * kAtKs * sizeof(float);
    if (!g_attn_attr_set[0]) {
      hipFuncSetAttribute(reinterpret_cast<const void*>(attn_tile_kernel<0>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      g_attn_attr_set[0] = true;
    }
    hipLaunchKernelGGL(attn_tile_kernel<0>, grid, dim3(256), lds, s, n_rows, tile_ptr, tile_col, tile_bits, q, k, v,
                       ld, scale, out, ldo, range_flag);
  } else {
    const size_t lds = (2 * kAtTile * kAtKh + 2 * kAtHead * kAtVt) * sizeof(unsigned short);
    if (!g_attn_attr_set[1]) {
      hipFuncSetAttribute(reinterpret_cast<const void*>(attn_tile_kernel<1>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      g_attn_attr_set[1] = true;
    }
    hipLaunchKernelGGL(attn_tile_kernel<1>, grid, dim3(256), lds, s, n_rows, tile_ptr, tile_col, tile_bits, q, k, v,
                       ld, scale, out, ldo, range_flag);
  }
  return check_launch("attn_tile_kernel");
}

int gc_ln_cond_rows(int n_rows, int rows_per_batch, const float* x, const float* scale, const float* offset,
                    float* out, void* stream) {
  if (n_rows <= 0 || rows_per_batch <= 0) return fail(GC_EINVAL, "gc_ln_cond_rows: bad sizes");
  if (!x || !scale || !offset || !out) return fail(GC_EINVAL, "gc_ln_cond_rows: null pointer");
  if ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(scale) | reinterpret_cast<size_t>(offset) |
       reinterpret_cast<size_t>(out)) & 15)
    return fail(GC_EINVAL, "gc_ln_cond_rows: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(ln_cond_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), n_rows,
                     rows_per_batch, x, scale, offset, out);
  return check_launch("ln_cond_kernel");
}

int gc_gelu_rows(long long n, float* x, void* stream) {
  if (n <= 0 || (n & 3)) return fail(GC_EINVAL, "gc_gelu_rows: n must be a positive multiple of 4");
  if (!x || (reinterpret_cast<size_t>(x) & 15)) return fail(GC_EINVAL, "gc_gelu_rows: x must be 16-byte aligned");
  const long n4 = (long)(n / 4);
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     n4, x);
  return check_launch("gelu_kernel");
}

int gc_permute_rows(int n, int batch, const int* idx, const float* src, long long src_bstride, int ld_src, float* dst,
                    long long dst_bstride, int ld_dst, void* stream) {
  if (n < 0 || batch <= 0 || batch > 65535) return fail(GC_EINVAL, "gc_permute_rows: bad sizes");
  if (n == 0) return 0;
  if (!idx || !src || !dst) return fail(GC_EINVAL, "gc_permute_rows: null pointer");
  if ((ld_src & 3) || (ld_dst & 3) || ((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) & 15))
    return fail(GC_EINVAL, "gc_permute_rows: rows must be 16-byte aligned");
  hipLaunchKernelGGL(permute_rows_kernel, dim3(n, batch), dim3(kD / 4), 0, static_cast<hipStream_t>(stream), n, idx,
                     src, (long)src_bstride, ld_src, dst, (long)dst_bstride, ld_dst);
  return check_launch("permute_rows_kernel");
}

}  // extern "C"
