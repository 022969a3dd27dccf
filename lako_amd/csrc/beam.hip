// Beam search on the device (FiDT5.generate(num_beams = K > 1); the semantics are those of transformers 5.15 `_beam_search`,
// restated in include/lako_hip.h).  A decode step ends in three launches instead of lako_greedy_step / lako_sample_step:
//   lako_beam_rows    per decoder row: log-softmax statistics and the row's 2K best tokens, sorted            (B·K workgroups)
//   lako_beam_merge   per question: the 2K best of its K·2K candidates, next running beams, finished set     (B workgroups)
//   lako_beam_gather  the self-attention K/V cache of every layer, rows reordered by parent beam              (streaming copy)
// Every order is fixed (thread-ordered partial sums, integer histograms, ranks by comparison) and there is no float atomic: the same
// input gives the same bits on every launch.  No allocation, no synchronisation: all three may be captured into a graph.
#include "common.h"

namespace {

constexpr int BR_T = 1024;       // lako_beam_rows: threads per row
constexpr int BM_T = 256;        // lako_beam_merge: threads per question
constexpr int BEAM_MAX_K = 16;
constexpr int BEAM_MAX_C = 2 * BEAM_MAX_K;

// x > y ⟺ key(x) > key(y) for non-NaN x, y (NaN and −0 are canonicalised by the reader)
__device__ __forceinline__ uint32_t beam_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float beam_canon(float x) { return x != x ? -INFINITY : (x == 0.f ? 0.f : x); }

// exclusive prefix of v over the workgroup's threads in thread order
__device__ __forceinline__ uint32_t beam_scan(uint32_t v, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < BR_T / 64; ++w)
    if (w < wave) base += wsum[w];
  __syncthreads();
  return base + inc - v;
}

// ---- lako_beam_rows ---------------------------------------------------------------------------------------------------------
// One workgroup per decoder row r.  The row is read from HBM once into LDS (V·4 bytes next to 1.5 KB of statics; LDSROW = false: it
// does not fit and every pass re-reads it from L2).  Thread t owns the contiguous indices [t·CH, (t+1)·CH), CH odd (conflict-free
// strides), so that index order is thread order.  The C-th largest key comes from a radix select over the order-preserving integer
// image of x, four passes of 8 bits with a COUNT histogram; the C kept entries — key > threshold, or equal to it up to the index
// where the count is reached — are compacted in index order and ranked by comparison (C <= 32): no sort of the row.
struct BeamRowsArgs {
  const float* logits;
  int64_t V;
  const float* run;
  float* cand_acc;
  int32_t* cand_tok;
  int C;
};

template <bool LDSROW>
__global__ __launch_bounds__(BR_T) void beam_rows_kernel(BeamRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char beam_smem[];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[BR_T / 64];
  __shared__ uint32_t sel[2];
  __shared__ float fred[2][BR_T / 64];
  __shared__ int pick;
  __shared__ uint32_t kkey[BEAM_MAX_C];
  __shared__ int kidx[BEAM_MAX_C];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = (int)a.V, C = a.C;
  const float* g = a.logits + (int64_t)r * a.V;
  float* row = reinterpret_cast<float*>(beam_smem);
  auto get = [&](int i) { return LDSROW ? row[i] : beam_canon(g[i]); };
  const int CH = ((V + BR_T - 1) / BR_T) | 1;
  const int i0 = (int)min((int64_t)V, (int64_t)tid * CH), i1 = (int)min((int64_t)V, (int64_t)tid * CH + CH);

  // ---- the row (once from HBM), its maximum and Σ exp(x − m): the statistics of lako_sample_step's score, in its order ------------
  float m = -INFINITY;
  for (int i = tid; i < V; i += BR_T) {
    const float x = beam_canon(g[i]);
    if (LDSROW) row[i] = x;
    m = fmaxf(m, x);
  }
  m = wave_max(m);
  if (lane == 0) fred[0][wave] = m;
  __syncthreads();
  m = fred[0][0];
#pragma unroll
  for (int w = 1; w < BR_T / 64; ++w) m = fmaxf(m, fred[0][w]);
  float se = 0.f;
  if (m > -INFINITY)
    for (int i = i0; i < i1; ++i) se += __expf(get(i) - m);
  se = wave_sum(se);
  if (lane == 0) fred[1][wave] = se;      // read after the barriers below

  // ---- the key of the C-th largest entry, and how many entries with exactly that key are still wanted -----------------------------
  uint32_t prefix = 0, pmask = 0, need = (uint32_t)C;
  for (int sh = 24; sh >= 0; sh -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    int cur = -1;
    uint32_t acc = 0;
    for (int i = i0; i < i1; ++i) {
      const uint32_t key = beam_key(get(i));
      if ((key & pmask) != prefix) continue;
      const int d = (int)((key >> sh) & 255u);
      if (d != cur) {      // a thread merges runs of equal digits before it adds
        if (acc) atomicAdd(&hist[cur], acc);
        cur = d;
        acc = 0;
      }
      ++acc;
    }
    if (acc) atomicAdd(&hist[cur], acc);
    __syncthreads();
    if (wave == 0) {
      const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const uint32_t s = h0 + h1 + h2 + h3;
      uint32_t inc = s;      // Σ over the lanes >= this one: the bins from the largest digit down
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_down(inc, o, 64);
        if (lane + o < 64) inc += n;
      }
      const uint32_t above = inc - s;
      if (lane == 0 && need > inc) {      // cannot happen (C <= V by the entry's check): keep the walk defined
        sel[0] = 0;
        sel[1] = 1;
      }
      if (above < need && need <= inc) {
        uint32_t rem = need - above;
        int d;
        if (rem <= h3) d = 3;
        else {
          rem -= h3;
          if (rem <= h2) d = 2;
          else {
            rem -= h2;
            if (rem <= h1) d = 1;
            else { rem -= h1; d = 0; }
          }
        }
        sel[0] = (uint32_t)(4 * lane + d);
        sel[1] = rem;
      }
    }
    __syncthreads();
    prefix |= sel[0] << sh;
    pmask |= 255u << sh;
    need = sel[1];
  }
  const uint32_t thr = prefix;

  // ---- the index of the need-th entry, ascending, whose key equals the threshold: equal values go by ascending index ---------------
  uint32_t c = 0;
  for (int i = i0; i < i1; ++i) c += beam_key(get(i)) == thr ? 1u : 0u;
  uint32_t ex = beam_scan(c, wsum);
  if (tid == 0) pick = V - 1;
  __syncthreads();
  if (ex < need && need <= ex + c) {
    uint32_t left = need - ex;
    for (int i = i0; i < i1; ++i)
      if (beam_key(get(i)) == thr && --left == 0) { pick = i; break; }
  }
  __syncthreads();
  const int cut = pick;

  // ---- the C kept entries, in index order ---------------------------------------------------------------------------------------
  c = 0;
  for (int i = i0; i < i1; ++i) {
    const uint32_t key = beam_key(get(i));
    c += (key > thr || (key == thr && i <= cut)) ? 1u : 0u;
  }
  ex = beam_scan(c, wsum);
  for (int i = i0; i < i1 && c; ++i) {
    const uint32_t key = beam_key(get(i));
    if (key > thr || (key == thr && i <= cut)) {
      if (ex < (uint32_t)C) {
        kkey[ex] = key;
        kidx[ex] = i;
      }
      ++ex;
      --c;
    }
  }
  __syncthreads();
  if (tid < C) {
    const uint32_t key = kkey[tid];
    int rank = 0;
    for (int j = 0; j < C; ++j) rank += (kkey[j] > key || (kkey[j] == key && j < tid)) ? 1 : 0;
    float s = fred[1][0];
#pragma unroll
    for (int w = 1; w < BR_T / 64; ++w) s += fred[1][w];
    const int i = kidx[tid];
    const float x = get(i);
    const float lp = x > -INFINITY ? (x - m) - __logf(s) : -INFINITY;
    a.cand_acc[(int64_t)r * C + rank] = a.run[r] + lp;
    a.cand_tok[(int64_t)r * C + rank] = i;
  }
}

// ---- lako_beam_merge ----------------------------------------------------------------------------------------------------------
// One workgroup per question b.  Its K·2K candidates are ranked by comparison (acc descending, then row, then token: the flat index
// k·V + v ascending); thread 0 walks the best 2K in order and decides the next running beams and the finished set; then all threads
// copy the token rows from the source set into the destination set (never in place: a permutation that swaps two beams would
// corrupt both).
struct BeamMergeArgs {
  const float* cand_acc;
  const int32_t* cand_tok;
  const int64_t* seq_src;
  int64_t* seq_dst;
  const int64_t* fin_src;
  int64_t* fin_dst;
  int64_t seq_ld;
  float* run;
  int64_t* next_ids;
  int32_t* parent;
  float* fin_score;
  float* fin_raw;
  int32_t* fin_len;
  uint8_t* fin_filled;
  uint8_t* open;
  int32_t* n_done;
  const uint32_t* params;
  int64_t eos, pad;
  int K, pos, last;
};

__global__ __launch_bounds__(BM_T) void beam_merge_kernel(BeamMergeArgs a) {
  __shared__ float cacc[BEAM_MAX_K * BEAM_MAX_C];
  __shared__ int ctok[BEAM_MAX_K * BEAM_MAX_C];
  __shared__ int top[BEAM_MAX_C];
  __shared__ int run_src[BEAM_MAX_K];      // candidate each new running beam is
  __shared__ int fin_from[BEAM_MAX_K];     // new finished slot j: old slot i (>= 0), or candidate c as −1 − c
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, C = 2 * K, n = K * C, pos = a.pos;
  const int64_t ld = a.seq_ld;
  for (int i = tid; i < n; i += BM_T) {
    const float v = a.cand_acc[(int64_t)b * n + i];
    cacc[i] = v != v ? -INFINITY : v;
    ctok[i] = a.cand_tok[(int64_t)b * n + i];
  }
  __syncthreads();
  for (int i = tid; i < n; i += BM_T) {
    const uint32_t key = beam_key(cacc[i]);
    const int ki = i / C, ti = ctok[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t kj = beam_key(cacc[j]);
      const int rj = j / C, tj = ctok[j];
      rank += (kj > key || (kj == key && (rj < ki || (rj == ki && tj < ti)))) ? 1 : 0;
    }
    if (rank < C) top[rank] = i;
  }
  __syncthreads();
  if (tid == 0) {
    const float lpen = __uint_as_float(a.params[0]);
    const bool early = a.params[1] != 0;
    const float norm = powf((float)pos, lpen);      // n = pos generated tokens
    float fs[BEAM_MAX_K], fr[BEAM_MAX_K];
    int fl[BEAM_MAX_K], ff[BEAM_MAX_K], from[BEAM_MAX_K];
    bool all_filled = true;
#pragma unroll
    for (int k = 0; k < BEAM_MAX_K; ++k) {
      if (k < K) {
        fs[k] = a.fin_score[b * K + k];
        fr[k] = a.fin_raw[b * K + k];
        fl[k] = a.fin_len[b * K + k];
        ff[k] = a.fin_filled[b * K + k];
        from[k] = k;
        all_filled = all_filled && ff[k];
      }
    }
    bool is_open = a.open[b] != 0;
    const bool accept = is_open && !(early && all_filled);
    int nrun = 0;
    for (int j = 0; j < C; ++j) {
      const int c = top[j];
      const bool ends = ctok[c] == (int)a.eos || a.last;
      if (!ends) {
        if (nrun < K) run_src[nrun++] = c;
      } else if (j < K && accept) {
        // insert behind every old or earlier entry that is at least as good (old before new on ties); an unfilled slot is worse than anything
        const float sc = cacc[c] / norm;
        int at = K;
#pragma unroll
        for (int k = BEAM_MAX_K - 1; k >= 0; --k)
          if (k < K && (!ff[k] || sc > fs[k])) at = k;
#pragma unroll
        for (int k = BEAM_MAX_K - 1; k >= 0; --k) {
          if (k < K && k > at) { fs[k] = fs[k - 1]; fr[k] = fr[k - 1]; fl[k] = fl[k - 1]; ff[k] = ff[k - 1]; from[k] = from[k - 1]; }
        }
#pragma unroll
        for (int k = 0; k < BEAM_MAX_K; ++k)
          if (k == at) { fs[k] = sc; fr[k] = cacc[c]; fl[k] = pos + 1; ff[k] = 1; from[k] = -1 - c; }
      }
    }
    // (the last step: every candidate ends and nothing runs on; keep the rows defined)
    for (int j = 0; nrun < K; ++j) run_src[nrun++] = top[j];
    all_filled = true;
    float worst = INFINITY;
#pragma unroll
    for (int k = 0; k < BEAM_MAX_K; ++k) {
      if (k < K) {
        a.fin_score[b * K + k] = fs[k];
        a.fin_raw[b * K + k] = fr[k];
        a.fin_len[b * K + k] = fl[k];
        a.fin_filled[b * K + k] = (uint8_t)ff[k];
        fin_from[k] = from[k];
        all_filled = all_filled && ff[k];
        worst = fminf(worst, fs[k]);
      }
    }
    const float best_run = cacc[run_src[0]];
    if (all_filled && best_run / norm <= worst) is_open = false;
    a.open[b] = is_open ? 1 : 0;
    if (!is_open || (early && all_filled) || a.last) atomicAdd(a.n_done, K);      // == B·K exactly when decoding has ended
  }
  __syncthreads();
  // ---- running beams: scores, next ids, parents, token rows ----------------------------------------------------------------------
  if (tid < K) {
    const int c = run_src[tid];
    a.run[b * K + tid] = cacc[c];
    a.next_ids[b * K + tid] = ctok[c];
    a.parent[b * K + tid] = b * K + c / C;
  }
  for (int e = tid; e < K * (pos + 1); e += BM_T) {
    const int k = e / (pos + 1), p = e % (pos + 1), c = run_src[k];
    a.seq_dst[(int64_t)(b * K + k) * ld + p] = p < pos ? a.seq_src[(int64_t)(b * K + c / C) * ld + p] : (int64_t)ctok[c];
  }
  // ---- finished set: whole rows (pad behind the end) -------------------------------------------------------------------------------
  for (int64_t e = tid; e < (int64_t)K * ld; e += BM_T) {
    const int k = (int)(e / ld), p = (int)(e % ld), f = fin_from[k];
    int64_t v;
    if (f >= 0) v = a.fin_src[(int64_t)(b * K + f) * ld + p];
    else {
      const int c = -1 - f;
      v = p < pos ? a.seq_src[(int64_t)(b * K + c / C) * ld + p] : (p == pos ? (int64_t)ctok[c] : a.pad);
    }
    a.fin_dst[(int64_t)(b * K + k) * ld + p] = v;
  }
}

// ---- lako_beam_gather -----------------------------------------------------------------------------------------------------------
// dst[l][r][p][off … off + width) = src[l][parent[r]][p][off … off + width) for p < n_pos, in 16-byte vectors; all strides in bytes.
__global__ __launch_bounds__(256) void beam_gather_kernel(const char* __restrict__ src, char* __restrict__ dst, const int32_t* __restrict__ parent,
                                                           int64_t layer_b, int64_t row_b, int64_t pos_b, int64_t off_b, int w16, int n_pos) {
  const int r = blockIdx.y, l = blockIdx.z;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_pos * w16) return;
  const int p = (int)(e / w16), c = (int)(e % w16);
  const int pr = parent[r];
  if ((unsigned)pr >= gridDim.y) return;      // not a row: leave the destination alone
  const int64_t in = l * layer_b + (int64_t)pr * row_b + p * pos_b + off_b + (int64_t)c * 16;
  const int64_t out = l * layer_b + (int64_t)r * row_b + p * pos_b + off_b + (int64_t)c * 16;
  *reinterpret_cast<uint4*>(dst + out) = *reinterpret_cast<const uint4*>(src + in);
}

}  // namespace

extern "C" int lako_beam_rows(const float* logits, int64_t V, int rows, int n_cand, const float* run, float* cand_acc, int32_t* cand_tok,
                              lako_stream_t stream) {
  LAKO_CHECK_ARG(logits && run && cand_acc && cand_tok, "lako_beam_rows: null operand");
  LAKO_CHECK_ARG(rows > 0 && V > 0 && V < (1ll << 30) && n_cand >= 1 && n_cand <= BEAM_MAX_C && n_cand <= V,
                 "lako_beam_rows: bad dims (rows=%d V=%lld n_cand=%d: 1 <= n_cand <= min(%d, V))", rows, (long long)V, n_cand, BEAM_MAX_C);
  BeamRowsArgs a{logits, V, run, cand_acc, cand_tok, n_cand};
  const size_t row_b = ((size_t)V * 4 + 15) & ~(size_t)15;
  if (row_b + 4096 <= 160 * 1024) {      // the row next to the static histogram / scan slots
    static lako_lds_cur_t cur;
    lako_raise_max_lds(reinterpret_cast<const void*>(&beam_rows_kernel<true>), (int)row_b, cur);
    hipLaunchKernelGGL((beam_rows_kernel<true>), dim3(rows), dim3(BR_T), row_b, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL((beam_rows_kernel<false>), dim3(rows), dim3(BR_T), 0, (hipStream_t)stream, a);
  }
  LAKO_LAUNCH_CHECK();
  return LAKO_OK;
}

extern "C" int lako_beam_merge(const float* cand_acc, const int32_t* cand_tok, int B, int K, const int64_t* seq_src, int64_t* seq_dst,
                               const int64_t* fin_src, int64_t* fin_dst, int64_t seq_ld, int pos, int last, float* run, int64_t* next_ids,
                               int32_t* parent, float* fin_score, float* fin_raw, int32_t* fin_len, uint8_t* fin_filled, uint8_t* open,
                               int32_t* n_done, const void* params, int64_t eos_id, int64_t pad_id, lako_stream_t stream) {
  LAKO_CHECK_ARG(cand_acc && cand_tok && seq_src && seq_dst && fin_src && fin_dst && run && next_ids && parent && fin_score && fin_raw &&
                 fin_len && fin_filled && open && n_done && params, "lako_beam_merge: null operand");
  LAKO_CHECK_ARG(B > 0 && K >= 1 && K <= BEAM_MAX_K && pos >= 1 && pos < seq_ld && (int64_t)B * K < (1ll << 24),
                 "lako_beam_merge: bad dims (B=%d K=%d pos=%d seq_ld=%lld: 1 <= K <= %d, 1 <= pos < seq_ld)", B, K, pos, (long long)seq_ld,
                 BEAM_MAX_K);
  LAKO_CHECK_ARG(seq_src != seq_dst && fin_src != fin_dst, "lako_beam_merge: the token rows are not updated in place");
  LAKO_CHECK_ALIGN(params, 4);
  BeamMergeArgs a{};
  a.cand_acc = cand_acc; a.cand_tok = cand_tok; a.seq_src = seq_src; a.seq_dst = seq_dst; a.fin_src = fin_src; a.fin_dst = fin_dst;
  a.seq_ld = seq_ld; a.run = run; a.next_ids = next_ids; a.parent = parent; a.fin_score = fin_score; a.fin_raw = fin_raw;
  a.fin_len = fin_len; a.fin_filled = fin_filled; a.open = open; a.n_done = n_done; a.params = (const uint32_t*)params;
  a.eos = eos_id; a.pad = pad_id; a.K = K; a.pos = pos; a.last = last ? 1 : 0;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(BM_T), 0, (hipStream_t)stream, a);
  LAKO_LAUNCH_CHECK();
  return LAKO_OK;
}

extern "C" int lako_beam_gather(const void* src, void* dst, const int32_t* parent, int layers, int rows, int n_pos, int64_t layer_bytes,
                                int64_t row_bytes, int64_t pos_bytes, int64_t off_bytes, int64_t width_bytes, lako_stream_t stream) {
  LAKO_CHECK_ARG(src && dst && parent && src != dst, "lako_beam_gather: null operand, or src == dst");
  LAKO_CHECK_ARG(layers > 0 && layers < 65536 && rows > 0 && rows < 65536 && n_pos > 0 && width_bytes > 0 && off_bytes >= 0 &&
                 off_bytes + width_bytes <= pos_bytes && (int64_t)n_pos * pos_bytes <= row_bytes && (int64_t)rows * row_bytes <= layer_bytes &&
                 width_bytes < (1ll << 30),
                 "lako_beam_gather: bad dims (layers=%d rows=%d n_pos=%d)", layers, rows, n_pos);
  LAKO_CHECK_ARG(((layer_bytes | row_bytes | pos_bytes | off_bytes | width_bytes) & 15) == 0, "lako_beam_gather: every size is a multiple of 16 bytes");
  LAKO_CHECK_ALIGN(src, 16);
  LAKO_CHECK_ALIGN(dst, 16);
  const int w16 = (int)(width_bytes / 16);
  const int64_t per_row = (int64_t)n_pos * w16;
  LAKO_CHECK_ARG(per_row < (1ll << 38), "lako_beam_gather: row too long");
  hipLaunchKernelGGL(beam_gather_kernel, dim3((unsigned)((per_row + 255) / 256), rows, layers), dim3(256), 0, (hipStream_t)stream,
                     (const char*)src, (char*)dst, parent, layer_bytes, row_bytes, pos_bytes, off_bytes, w16, n_pos);
  LAKO_LAUNCH_CHECK();
  return LAKO_OK;
}
