// rk_screen_abund.inc -- the device side of rk_screen_abund_rows that rk_screen_rows does not have, included by rk_screen.hip inside its
// namespace (Key, better, wave_best, Walk and the constants are its): the fill kernel and the two select kernels.  include/rabbitkssd.h,
// the screen with abundances; DESIGN.md 4.20.
//
// After the write kernel of a batch (its second instantiation) map[slot][ref] = the record of that cell within the batch + 1 (0: none)
// lies where the won row was, seg[record] = where the record's `common` values begin within its sub-range of rows, and cur[2 record],
// cur[2 record + 1] = 0 are its front and back cursors.
//   fill     k_screen_fill: the tiles, the slot search, the look-up and the three walks of k_screen_win, every list walked twice: first
//            for its winner, as k_screen_win finds it, then to hand the count m of the hash to every holder whose cell has a record --
//            the winner's at seg + front++, everybody else's at seg + common - 1 - back++.  Also the three sums of m per query row;
//   select   k_screen_select_wave, one wave per record: up to kRankMax values are ranked in registers (every lane one value, n shuffles),
//            up to wave_sel_max by a radix select in the wave's own pair of LDS histograms; k_screen_select_block, one workgroup per
//            longer record, the same radix select with kScreenThreads values per step.
// Memory scope: as rk_screen.hip.  Inside a launch workgroups meet only in relaxed agent-scope adds (the cursors, the sums, the
// statistics); a cursor's returned value places a store, nothing reads another workgroup's store before the launch is over.

constexpr uint32_t kRankMax = 64;          // the longest segment a wave ranks in registers: one value per lane
constexpr uint32_t kWaveSelMax = 2048;     // the longest segment one wave selects by radix (32 values per lane and round)
static_assert(sizeof(rk_screen_abund) == 24 && sizeof(rk_screen_abund_stats) == 176, "the layouts of include/rabbitkssd.h");
static_assert(kRankMax == 64 && kRankMax < kWaveSelMax, "the classes of segment lengths");

struct AbundCounters {   // one device block for the whole call
    unsigned long long rank_segs, wave_segs, block_segs;
    unsigned long long errors;   // a cursor beyond its segment, a segment beyond the values: the host reports an internal error
};

struct FillArgs {
    const void *q_hashes;              // Hash[total]
    const uint32_t *q_counts;          // u32[total]
    const uint64_t *q_off;             // u64[Q + 1]
    const uint32_t *row_of;            // the sub-range: slot s is query row row_of[s]
    const unsigned long long *hoff;    // nb + 1
    uint32_t nb;
    unsigned long long n_hashes;
    IndexLookup ix;
    const uint32_t *postings, *upos, *orig, *sizes_internal;
    const int32_t *cnt;                // [nb][n_ref]
    const uint32_t *map;               // [nb][n_ref]: the record of the cell within the batch + 1
    uint32_t n_ref, min_common, lane_max, wave_max;
    const unsigned long long *seg;     // per record of the batch
    uint32_t *cur;                     // two per record of the batch
    uint32_t *vals;
    unsigned long long vals_cap;       // entries of vals
    unsigned long long *occ_q;         // three per QUERY row
    AbundCounters *c;
};

// the count m of a hash of slot `slot` goes to the holder at postings[at], if its cell has a record
__device__ __forceinline__ void deposit(const FillArgs &a, uint32_t at, uint32_t slot, uint32_t m, const Key &win)
{
    const uint32_t p = a.postings[at];
    const uint32_t r = a.orig ? a.orig[p] : p;
    const size_t cell = (size_t)slot * a.n_ref + r;
    const uint32_t rec1 = a.map[cell];
    if (!rec1) return;
    const uint32_t rec = rec1 - 1, common = (uint32_t)a.cnt[cell];
    const bool claimed = win.c && win.r == r;
    const uint32_t k = __hip_atomic_fetch_add(a.cur + 2 * (size_t)rec + (claimed ? 0 : 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long pos = a.seg[rec] + (claimed ? k : common - 1 - k);
    if (k >= common || pos >= a.vals_cap) {   // (never: a cell is visited once per shared hash, the segments lie within the values)
        add_u64(&a.c->errors, 1);
        return;
    }
    a.vals[pos] = m;
}

template <class Hash> __global__ void __launch_bounds__(kScreenThreads) k_screen_fill(FillArgs a)
{
    __shared__ uint32_t s_qn[kTrips], s_qbeg[kScreenThreads], s_qlen[kScreenThreads], s_qslot[kScreenThreads], s_qm[kScreenThreads];
    __shared__ Key s_part[kScreenThreads][kWaves];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < (uint32_t)kTrips) s_qn[tid] = 0;
    const unsigned long long base = (unsigned long long)blockIdx.x * kTileHashes + (unsigned long long)wave * (kTrips * 64);
    const Hash *q = (const Hash *)a.q_hashes;
    const unsigned long long h0 = a.hoff[0];
    uint32_t slo[kTrips], shi[kTrips];
    bool in[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        in[t] = base + 64 * t + lane < a.n_hashes;
        slo[t] = 0;
        shi[t] = in[t] ? a.nb - 1 : 0u;
    }
    for (bool more = true; more;) {   // the slot of every hash: as k_screen_win
        more = false;
#pragma unroll
        for (int t = 0; t < kTrips; t++)
            if (slo[t] < shi[t]) {
                const uint32_t mid = slo[t] + (shi[t] - slo[t] + 1) / 2;
                if (a.hoff[mid] - h0 <= base + 64 * t + lane) slo[t] = mid; else shi[t] = mid - 1;
                more |= slo[t] < shi[t];
            }
    }
    unsigned long long h[kTrips];
    uint32_t list[kTrips], mult[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        h[t] = 0;
        mult[t] = 0;
        if (in[t]) {
            const uint32_t row = a.row_of[slo[t]];
            const unsigned long long at = a.q_off[row] + (base + 64 * t + lane - (a.hoff[slo[t]] - h0));
            h[t] = (unsigned long long)q[at];
            mult[t] = a.q_counts[at];
        }
    }
    index_lookup<Hash, kTrips>(a.ix, h, in, list);
    __syncthreads();   // (s_qn)
#pragma unroll
    for (int t = 0; t < kTrips; t++) {
        const uint32_t slot = slo[t], m = mult[t];
        uint32_t beg = 0, len = 0;
        if (list[t] != kNoList) {
            beg = a.upos[list[t]];
            len = a.upos[list[t] + 1] - beg;
        }
        const bool found = len > 0;
        const bool by_lane = found && len <= a.lane_max, by_wave = found && !by_lane && len <= a.wave_max, by_block = found && !by_lane && !by_wave;
        Key win{0, 0, 0};
        if (by_lane) {
            Walk wk{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)slot * a.n_ref, a.min_common};
            for (uint32_t j = 0; j < len; j++) wk.see(beg + j, &win);
            for (uint32_t j = 0; j < len; j++) deposit(a, beg + j, slot, m, win);
        }
        unsigned long long pending = __ballot(by_wave);
        while (pending) {   // (uniform in the wave)
            const int src = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const uint32_t b = (uint32_t)__shfl((int)beg, src), l = (uint32_t)__shfl((int)len, src), sl = (uint32_t)__shfl((int)slot, src),
                           mm = (uint32_t)__shfl((int)m, src);
            Walk ww{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)sl * a.n_ref, a.min_common};
            Key mine{0, 0, 0};
            for (uint32_t j = lane; j < l; j += 64) ww.see(b + j, &mine);
            mine = wave_best(mine);
            for (uint32_t j = lane; j < l; j += 64) deposit(a, b + j, sl, mm, mine);
            if (lane == src) win = mine;
        }
        uint32_t at = 0;
        if (by_block) {
            at = atomicAdd(&s_qn[t], 1u);   // (at most one per thread and trip: at < kScreenThreads)
            s_qbeg[at] = beg;
            s_qlen[at] = len;
            s_qslot[at] = slot;
            s_qm[at] = m;
        }
        __syncthreads();
        const uint32_t qn = s_qn[t];
        if (qn) {   // (uniform in the workgroup)
            for (uint32_t k = 0; k < qn; k++) {
                Walk wb{a.postings, a.orig, a.sizes_internal, a.cnt + (size_t)s_qslot[k] * a.n_ref, a.min_common};
                const uint32_t b = s_qbeg[k], l = s_qlen[k];
                Key mine{0, 0, 0};
                for (uint32_t j = tid; j < l; j += kScreenThreads) wb.see(b + j, &mine);
                mine = wave_best(mine);
                if (lane == 0) s_part[k][wave] = mine;
            }
            __syncthreads();
            for (uint32_t k = 0; k < qn; k++) {
                Key w = s_part[k][0];
#pragma unroll
                for (int v = 1; v < kWaves; v++)
                    if (better(s_part[k][v], w)) w = s_part[k][v];
                const uint32_t b = s_qbeg[k], l = s_qlen[k], sl = s_qslot[k], mm = s_qm[k];
                for (uint32_t j = tid; j < l; j += kScreenThreads) deposit(a, b + j, sl, mm, w);
                if (by_block && at == k) win = w;
            }
            __syncthreads();   // (the queue and the partial keys are free for the next trip)
        }
        // the sums of the row: the equal slots of a run of 64 hashes are added once per wave
        {
            unsigned long long todo = __ballot(in[t]);
            while (todo) {   // (uniform)
                const int lead = __ffsll((long long)todo) - 1;
                const uint32_t sl = (uint32_t)__shfl((int)slot, lead);
                const bool same = in[t] && slot == sl;
                const unsigned long long all = wave_sum(same ? m : 0u), mat = wave_sum(same && found ? m : 0u), cla = wave_sum(same && win.c ? m : 0u);
                if (lane == lead) {
                    unsigned long long *o = a.occ_q + 3 * (size_t)a.row_of[sl];
                    add_u64(o, all);
                    if (mat) add_u64(o + 1, mat);
                    if (cla) add_u64(o + 2, cla);
                }
                todo &= ~__ballot(same);
            }
        }
    }
}

struct SelArgs {
    const rk_screen_rec *recs;         // the records of the batch
    const unsigned long long *seg;
    const uint32_t *vals;
    unsigned long long vals_cap;
    rk_screen_abund *out;              // per record of the batch
    unsigned long long rec_first, rec_end;   // the records of the sub-range
    uint32_t wave_sel_max;
    AbundCounters *c;
};

// by a full wave: the bin of hist[256] that holds the entry of 0-based rank k, and the rank within that bin (k below the sum of hist)
__device__ __forceinline__ void find_bin(const uint32_t *hist, uint32_t k, int lane, uint32_t *bin, uint32_t *k_out)
{
    uint32_t c[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        c[i] = hist[4 * lane + i];
        s += c[i];
    }
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = (uint32_t)__shfl((int)incl, (lane - o) & 63);
        if (lane >= o) incl += x;
    }
    const uint32_t excl = incl - s;
    const unsigned long long m = __ballot(excl <= k && k < incl);
    const int owner = m ? __ffsll((long long)m) - 1 : 63;
    uint32_t kk = k - excl, b = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (b == (uint32_t)i && kk >= c[i]) {
            kk -= c[i];
            b = i + 1;
        }
    *bin = (uint32_t)__shfl((int)(4 * lane + b), owner);
    *k_out = (uint32_t)__shfl((int)kk, owner);
}

// the threads of a group of T (a wave: 64, the workgroup: kScreenThreads) meet; LDS written before is seen after
template <int T> __device__ __forceinline__ void group_sync()
{
    if constexpr (T == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// The sums and the lower medians of v[0 .. won) and v[0 .. n), n > 0, by a group of T threads of which this one is thread t: four
// rounds of 8 bits from the top, per round the histogram of the entries that agree with the bits found so far, for both parts at once.
// hist: 512 words of LDS of the group, bc: 4 words, red: 2 * T / 64 words of 64 bits.  Thread 0 of the group writes *out.
template <int T>
__device__ __forceinline__ void select_radix(const uint32_t *v, uint32_t n, uint32_t won, uint32_t *hist, uint32_t *bc, unsigned long long *red, int t,
                                             rk_screen_abund *out)
{
    uint32_t pre_a = 0, pre_w = 0, ka = (n - 1) / 2, kw = won ? (won - 1) / 2 : 0;
    unsigned long long sa = 0, sw = 0;
#pragma unroll 1
    for (int round = 0; round < 4; round++) {
        const int shift = 24 - 8 * round;
        for (int i = t; i < 512; i += T) hist[i] = 0;
        group_sync<T>();
        for (uint32_t i = t; i < n; i += T) {
            const uint32_t x = v[i];
            const uint32_t top = round ? x >> (shift + 8) : 0u, b = (x >> shift) & 255u;
            if (!round) {
                sa += x;
                if (i < won) sw += x;
            }
            if (top == pre_a) atomicAdd(&hist[b], 1u);
            if (i < won && top == pre_w) atomicAdd(&hist[256 + b], 1u);
        }
        group_sync<T>();
        if (t < 64) {   // (a whole wave)
            uint32_t bin_a, bin_w = 0, ka2, kw2 = 0;
            find_bin(hist, ka, t, &bin_a, &ka2);
            if (won) find_bin(hist + 256, kw, t, &bin_w, &kw2);   // (uniform)
            if (t == 0) {
                bc[0] = bin_a;
                bc[1] = ka2;
                bc[2] = bin_w;
                bc[3] = kw2;
            }
        }
        group_sync<T>();
        pre_a = (pre_a << 8) | bc[0];
        ka = bc[1];
        pre_w = (pre_w << 8) | bc[2];
        kw = bc[3];
        group_sync<T>();   // (bc and hist are rewritten by the next round)
    }
    sa = wave_sum(sa);
    sw = wave_sum(sw);
    if constexpr (T > 64) {
        if ((t & 63) == 0) {
            red[2 * (t >> 6)] = sa;
            red[2 * (t >> 6) + 1] = sw;
        }
        __syncthreads();
        sa = sw = 0;
        for (int k = 0; k < T / 64; k++) {
            sa += red[2 * k];
            sw += red[2 * k + 1];
        }
    }
    if (t == 0) *out = rk_screen_abund{sa, sw, pre_a, won ? pre_w : 0u};
}

// One wave per record of the sub-range: segments of up to kRankMax values ranked in registers, of up to wave_sel_max by radix
__global__ void __launch_bounds__(kScreenThreads) k_screen_select_wave(SelArgs a)
{
    __shared__ uint32_t s_hist[kWaves][512], s_bc[kWaves][4], s_cls[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long rec = a.rec_first + (unsigned long long)blockIdx.x * kWaves + wave;
    uint32_t cls = 0;   // 1: ranked, 2: radix
    if (rec < a.rec_end) {   // (uniform in the wave)
        const uint32_t n = a.recs[rec].common, won = a.recs[rec].won;
        const unsigned long long seg = a.seg[rec];
        if (!n || won > n || seg + n > a.vals_cap) {   // (never)
            if (lane == 0) add_u64(&a.c->errors, 1);
        } else if (n <= a.wave_sel_max) {
            const uint32_t *v = a.vals + seg;
            if (n <= kRankMax) {
                cls = 1;
                const uint32_t x = (uint32_t)lane < n ? v[lane] : 0u;
                uint32_t ra = 0, rw = 0;
                for (uint32_t j = 0; j < n; j++) {   // (uniform)
                    const uint32_t y = (uint32_t)__shfl((int)x, (int)j);
                    const uint32_t less = y < x || (y == x && j < (uint32_t)lane);
                    ra += less;
                    if (j < won) rw += less;
                }
                const unsigned long long sa = wave_sum(x), sw = wave_sum((uint32_t)lane < won ? x : 0u);
                const unsigned long long ma = __ballot((uint32_t)lane < n && ra == (n - 1) / 2);
                const unsigned long long mw = __ballot(won && (uint32_t)lane < won && rw == (won - 1) / 2);
                const uint32_t med_a = (uint32_t)__shfl((int)x, ma ? __ffsll((long long)ma) - 1 : 0);
                const uint32_t med_w = (uint32_t)__shfl((int)x, mw ? __ffsll((long long)mw) - 1 : 0);
                if (lane == 0) a.out[rec] = rk_screen_abund{sa, sw, med_a, won ? med_w : 0u};
            } else {
                cls = 2;
                select_radix<64>(v, n, won, s_hist[wave], s_bc[wave], nullptr, lane, a.out + rec);
            }
        }
    }
    if (lane == 0) s_cls[wave] = cls;
    __syncthreads();
    if (tid == 0) {
        uint32_t n_rank = 0, n_wave = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            n_rank += s_cls[k] == 1;
            n_wave += s_cls[k] == 2;
        }
        if (n_rank) add_u64(&a.c->rank_segs, n_rank);
        if (n_wave) add_u64(&a.c->wave_segs, n_wave);
    }
}

// One workgroup per record of the sub-range with more than wave_sel_max values
__global__ void __launch_bounds__(kScreenThreads) k_screen_select_block(SelArgs a)
{
    __shared__ uint32_t s_hist[512], s_bc[4];
    __shared__ unsigned long long s_red[2 * kWaves];
    const unsigned long long rec = a.rec_first + blockIdx.x;
    if (rec >= a.rec_end) return;   // (uniform)
    const uint32_t n = a.recs[rec].common, won = a.recs[rec].won;
    const unsigned long long seg = a.seg[rec];
    if (n <= a.wave_sel_max) return;   // (uniform: the wave kernel's)
    if (won > n || seg + n > a.vals_cap) {   // (uniform; never)
        if (threadIdx.x == 0) add_u64(&a.c->errors, 1);
        return;
    }
    select_radix<kScreenThreads>(a.vals + seg, n, won, s_hist, s_bc, s_red, (int)threadIdx.x, a.out + rec);
    if (threadIdx.x == 0) add_u64(&a.c->block_segs, 1);
}
