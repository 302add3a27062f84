// Stable segmented radix sort of fp32 keys with a 32-bit payload, descending by the key's bit pattern
// (numeric order for non-negative floats); equal keys keep their input order.  keys [Q][P]: every row is
// sorted on its own.  LSD, kSortBits-bit digits, 32 / kSortBits passes, three launches per pass:
//   sort_hist_kernel    grid (nblk, Q): digit histogram of one tile of kSortTile keys -> table[q][digit][blk]
//   sort_scan_kernel    grid (kSortBins, Q): exclusive scan of one digit's counts over the blocks (a loop with a
//                       carry, bound known at launch) and the digit's total -> dtot[q][digit]
//   sort_scatter_kernel grid (nblk, Q): stable rank of every key of the tile among the tile's keys of the same
//                       digit (per-wave counters in LDS, lanes of equal digit matched with 64-bit ballots),
//                       tile reordered by digit in LDS, then written in runs to
//                       scan(dtot)[digit] + table[q][digit][blk] + rank
// No block waits on another: every cross-block dependency is a launch boundary.  The only atomics are integer
// LDS counts of the histogram, whose result does not depend on arrival order.  Any bit pattern (negative, NaN)
// is ordered by its bits; positions come from counts of the same data, so every write stays inside the row.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSortBits = 8;
constexpr int kSortBins = 1 << kSortBits;
constexpr int kRounds = 16;                           // 64-key rounds per wave
constexpr int kWaveKeys = 64 * kRounds;               // consecutive keys owned by one wave
constexpr int kSortTile = kWaves * kWaveKeys;         // keys per block
static_assert(kSortBins == kBlock, "one thread per digit");

// descending order on the key bits == ascending order on their complement
DEVI unsigned sort_digit(unsigned key, int shift) { return (~key >> shift) & (kSortBins - 1); }

// exclusive scan of one value per thread over the block (kBlock threads, fixed order); total to every thread
DEVI unsigned block_excl_scan(unsigned v, unsigned* wsum, unsigned& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();   // wsum may still be read from an earlier call
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  unsigned off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const unsigned s = wsum[w];
    if (w < wv) off += s;
    tot += s;
  }
  total = tot;
  return off + inc - v;
}

__global__ __launch_bounds__(kBlock) void sort_hist_kernel(const unsigned* __restrict__ keys,
                                                           unsigned* __restrict__ table, long P, int nblk,
                                                           int shift) {
  __shared__ unsigned hist[kSortBins];
  const int q = blockIdx.y, blk = blockIdx.x;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* row = keys + (long)q * P;
  const long base = (long)blk * kSortTile;
#pragma unroll 4
  for (int r = 0; r < kSortTile / kBlock; ++r) {
    const long i = base + r * kBlock + threadIdx.x;
    if (i < P) atomicAdd(&hist[sort_digit(row[i], shift)], 1u);
  }
  __syncthreads();
  table[((long)q * kSortBins + threadIdx.x) * nblk + blk] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void sort_scan_kernel(unsigned* __restrict__ table, unsigned* __restrict__ dtot,
                                                           int nblk) {
  __shared__ unsigned wsum[kWaves];
  const int q = blockIdx.y, d = blockIdx.x;
  unsigned* row = table + ((long)q * kSortBins + d) * nblk;
  unsigned carry = 0;
  for (int base = 0; base < nblk; base += kBlock) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nblk ? row[i] : 0u;
    unsigned total;
    const unsigned ex = block_excl_scan(v, wsum, total);
    if (i < nblk) row[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) dtot[q * kSortBins + d] = carry;
}

// IOTA: the payload of the first pass is the key's position in its row
template <bool IOTA>
__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(const unsigned* __restrict__ kin,
                                                              const unsigned* __restrict__ pin,
                                                              unsigned* __restrict__ kout,
                                                              unsigned* __restrict__ pout,
                                                              const unsigned* __restrict__ table,
                                                              const unsigned* __restrict__ dtot, long P, int nblk,
                                                              int shift) {
  __shared__ unsigned cnt[kWaves][kSortBins];   // keys of a digit per wave, then the exclusive prefix over waves
  __shared__ unsigned boff[kSortBins];          // first slot of a digit in the reordered tile
  __shared__ unsigned gdst[kSortBins];          // row position of that slot (mod 2^32)
  __shared__ unsigned sk[kSortTile], sp[kSortTile];
  __shared__ unsigned wsum[kWaves];
  const int q = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long rowoff = (long)q * P, base = (long)blk * kSortTile;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) cnt[w][threadIdx.x] = 0;
  __syncthreads();

  unsigned key[kRounds], pay[kRounds], rank[kRounds];
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const long i = base + wv * kWaveKeys + r * 64 + lane;
    const bool valid = i < P;
    key[r] = valid ? kin[rowoff + i] : 0u;
    pay[r] = valid ? (IOTA ? (unsigned)i : pin[rowoff + i]) : 0u;
    const unsigned d = sort_digit(key[r], shift);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < kSortBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(valid && bit);
      m &= bit ? bal : ~bal;
    }
    if (!valid) m = 0;
    // the lowest lane of every group of equal digits takes the group's slots from the wave's counter
    const int leader = valid ? __ffsll((long long)m) - 1 : lane;
    unsigned old = 0;
    if (valid && lane == leader) {
      old = cnt[wv][d];
      cnt[wv][d] = old + (unsigned)__popcll(m);
    }
    rank[r] = __shfl(old, leader, 64) + (unsigned)__popcll(m & lt);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  {   // thread d: prefix of digit d over the waves, then over the digits
    const int d = threadIdx.x;
    unsigned tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const unsigned c = cnt[w][d];
      cnt[w][d] = tot;
      tot += c;
    }
    unsigned all;
    const unsigned ex = block_excl_scan(tot, wsum, all);
    const unsigned dbase = block_excl_scan(dtot[q * kSortBins + d], wsum, all);
    boff[d] = ex;
    gdst[d] = dbase + table[((long)q * kSortBins + d) * nblk + blk] - ex;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const long i = base + wv * kWaveKeys + r * 64 + lane;
    if (i < P) {
      const unsigned d = sort_digit(key[r], shift);
      const unsigned pos = boff[d] + cnt[wv][d] + rank[r];   // < number of valid keys of the tile
      sk[pos] = key[r];
      sp[pos] = pay[r];
    }
  }
  __syncthreads();
  const int nvalid = (int)(P - base < (long)kSortTile ? P - base : (long)kSortTile);
  for (int i = threadIdx.x; i < nvalid; i += kBlock) {
    const unsigned k = sk[i];
    const unsigned dst = gdst[sort_digit(k, shift)] + (unsigned)i;   // < P
    kout[rowoff + dst] = k;
    pout[rowoff + dst] = sp[i];
  }
}
}  // namespace

int sort_tile() { return kSortTile; }
int sort_bins() { return kSortBins; }
int sort_passes() { return 32 / kSortBits; }

void sort_segments(const unsigned* keys, const unsigned* payload, unsigned* out_keys, unsigned* out_payload,
                   unsigned* tmp_keys, unsigned* tmp_payload, unsigned* table, unsigned* dtot, int Q, long P,
                   hipStream_t s) {
  const int nblk = cdiv(P, kSortTile);
  const dim3 gt(nblk, Q), gs(kSortBins, Q);
  const unsigned *kin = keys, *pin = payload;
  constexpr int passes = 32 / kSortBits;   // even: the last pass lands in the output buffers
  static_assert(passes % 2 == 0, "ping-pong ends in the output");
  for (int p = 0; p < passes; ++p) {
    unsigned* ko = (p & 1) ? out_keys : tmp_keys;
    unsigned* po = (p & 1) ? out_payload : tmp_payload;
    const int shift = p * kSortBits;
    sort_hist_kernel<<<gt, kBlock, 0, s>>>(kin, table, P, nblk, shift);
    sort_scan_kernel<<<gs, kBlock, 0, s>>>(table, dtot, nblk);
    if (p == 0 && payload == nullptr)
      sort_scatter_kernel<true><<<gt, kBlock, 0, s>>>(kin, nullptr, ko, po, table, dtot, P, nblk, shift);
    else
      sort_scatter_kernel<false><<<gt, kBlock, 0, s>>>(kin, pin, ko, po, table, dtot, P, nblk, shift);
    kin = ko;
    pin = po;
  }
}
