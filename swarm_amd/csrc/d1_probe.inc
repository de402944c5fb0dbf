// d1_probe.inc — the plain probe of the d = 1 network: the wave-cooperative enumeration of a sequence's microvariants and
// the kernel template k_d1_probe that looks them up in the amplicon table.  Included once by d1.hip and once by
// fastidious.hip, inside the anonymous namespace, after wave_ops.inc, key_ops.inc and d1_common.inc.  A unit owns the MODEs
// it launches, and only those are instantiated in its code object:
//   d1.hip          MODE 0 (the network on the plain route) and MODE 2 (the seeds the anchored passes cannot serve);
//   fastidious.hip  MODE 1 (the second level of the Bloom route); k_d1_flex and k_fast_count there use enumerate_variants.

struct alignas(16) swa_task {   // one surviving first-level microvariant of a heavy amplicon
  uint64_t hash;
  uint32_t heavy;
  uint32_t code;
};

struct NetArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint64_t * abundance;
  const uint64_t * zobrist;     // 4 * zlen
  uint32_t zlen;
  uint32_t maxwords;            // ceil(longest / 32)
  const swa_slot * table;
  uint64_t tmask;
  const uint64_t * bloom;
  uint64_t bmask;
  const uint64_t * patterns;    // 1024
  int no_cluster_breaking;
  uint32_t first;
  uint32_t count;
  uint64_t * edges;             // (src << 32) | dst
  uint64_t seg_cap;             // edges are appended to per-wave segments: segment w = edges[w*seg_cap ..)
  uint32_t * seg_fill;          // [launch waves] fill of each segment (no atomics: one writer per segment)
  // MODE 2 (seeds the anchored passes cannot serve): explicit (seed, position range) list
  const struct swa_fallback * fallback;
  const uint32_t * fallback_count;
  const struct swa_aux * aux;
  // MODE 0 in a multi-GPU job (swa_d1_set_ownership, world > 1): only seeds with id mod world == rank
  uint32_t owner_rank, owner_world;
  // MODE 1 (fastidious second level)
  const swa_task * tasks;
  uint32_t * graft;
  unsigned long long * cand_counter;
  uint32_t fast_min_len;        // a (heavy, light) pair with both lengths in [fast_min_len, fast_max_len] belongs to the pair
  uint32_t fast_max_len;        // route (d1_fast.inc); every other pair is admitted here (no upper bound: 0xFFFFFFFF)
  // MODE 2 in window mode (anchor windows moved inwards): a fallback seed's share is defined by the window itself —
  // range 1 = neighbours with the same prefix-side window (word win_word), range 2 = the others; all positions are
  // enumerated and the hits filtered
  uint32_t window_mode, win_word;
  uint32_t anchor_w;            // width of the anchor windows in nt (32 / 64 / 128): the window is words [win_word, win_word + anchor_w / 32)
};

// Wave-cooperative enumeration of all microvariants of the staged sequence `sw` (len nt).
// Lane l owns positions [l*K, (l+1)*K), K = ceil((len+1)/64); `f(slots)` is called once
// per owned position (K times, wave-uniformly) with that position's 8 candidate slots:
//   [0..3] insertion of base b before p        (variants.cc:226-246)
//   [4..6] substitution of p by the 3 others   (variants.cc:192-206)
//   [7]    deletion of p, once per run          (variants.cc:210-222)
// code = type | base << 2 | pos << 4.  Returns the sequence's own hash.
struct Slots {
  uint64_t hs[8];
  bool ok[8];
  uint32_t code[8];
};

template <class F>
__device__ __forceinline__ uint64_t enumerate_variants(const uint64_t * sw, uint32_t len, const uint64_t * zob,
                                                       int lane, F && f) {
  // pass 1: per-lane XOR of the three Zobrist streams over the owned positions
  const uint32_t K = (len + 64u) >> 6;                     // ceil((len + 1) / 64)
  const uint32_t p0 = (uint32_t)lane * K;
  uint64_t xa = 0, xd = 0, xi = 0;
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t p = p0 + j;
    if (p < len) {
      const uint32_t c = swa_nt(sw, p);
      xa ^= zob[4u * p + c];
      if (p >= 1u) { xd ^= zob[4u * (p - 1u) + c]; }
      xi ^= zob[4u * (p + 1u) + c];
    }
  }
  // wave scans: exclusive prefix of xa; inclusive suffixes of xd, xi
  uint64_t pa = xa, sd = xd, si = xi;
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const uint64_t ta = swa_shfl_up_u64(pa, d);
    const uint64_t td = swa_shfl_down_u64(sd, d);
    const uint64_t ti = swa_shfl_down_u64(si, d);
    if (lane >= (int)d) { pa ^= ta; }
    if (lane + (int)d < 64) { sd ^= td; si ^= ti; }
  }
  const uint64_t H = swa_shfl_u64(pa, 63);                 // hash of the whole sequence
  pa ^= xa;                                                // exclusive

  // pass 2: the variants of the owned positions
  uint32_t prevc = (p0 >= 1u && p0 - 1u < len) ? swa_nt(sw, p0 - 1u) : 4u;
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t p = p0 + j;
    const bool in_seq = p < len;
    const bool in_ins = p <= len;
    const uint32_t c = in_seq ? swa_nt(sw, p) : 4u;
    uint64_t z[4];
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) { z[b] = in_ins ? zob[4u * p + b] : 0ull; }
    // z[c] without dynamic register indexing
    const uint64_t zc = (c == 0u) ? z[0] : (c == 1u) ? z[1] : (c == 2u) ? z[2] : z[3];
    const uint64_t za = in_seq ? zc : 0ull;
    const uint64_t zd = (in_seq && p >= 1u) ? zob[4u * (p - 1u) + c] : 0ull;
    const uint64_t zi = in_seq ? zob[4u * (p + 1u) + c] : 0ull;

    Slots s;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
      s.hs[b] = pa ^ z[b] ^ si;
      s.ok[b] = in_ins && (p == 0u || b != prevc);
      s.code[b] = 2u | (b << 2) | (p << 4);
    }
#pragma unroll
    for (uint32_t t = 0; t < 3u; ++t) {
      const uint32_t b = (t < c) ? t : t + 1u;               // the t-th base that is not c
      s.hs[4 + t] = H ^ za ^ ((t < c) ? z[t] : z[t + 1u]);
      s.ok[4 + t] = in_seq;
      s.code[4 + t] = 0u | (b << 2) | (p << 4);
    }
    s.hs[7] = pa ^ sd ^ zd;
    s.ok[7] = in_seq && (p == 0u || c != prevc);
    s.code[7] = 1u | (p << 4);

    f(s);

    // advance the running prefix / suffixes past position p
    pa ^= za;
    sd ^= zd;
    si ^= zi;
    prevc = c;
  }
  return H;
}

// Microvariants of positions [pb, pe) only (pe <= len + 1; position len carries insertions
// only).  H = hash of the sequence, baseA = XOR of Z[q][s_q] over q < pb, tailD / tailI = XOR
// of Z[q-1][s_q] / Z[q+1][s_q] over q >= pb.  Same slot layout as enumerate_variants.
// Written without data-dependent branches: every table read uses a clamped (always valid)
// index and validity travels as 0/1 integers, because on this kernel the CU's single scalar
// unit (exec-mask bookkeeping of divergent branches), not the vector ALUs, was the limiter.
struct SlotsI {
  uint64_t hs[8];
  uint32_t ok[8];       // 0 / 1
  uint32_t code[8];
};

template <class F>
__device__ __forceinline__ void enumerate_range(const uint64_t * sw, uint32_t len, const uint64_t * zob, int lane,
                                                uint32_t pb, uint32_t pe, uint64_t H, uint64_t baseA, uint64_t tailD,
                                                uint64_t tailI, F && f) {
  const uint32_t K = (pe - pb + 63u) >> 6;
  const uint32_t p0 = pb + (uint32_t)lane * K;
  const uint32_t lim = pe < len ? pe : len;                  // positions that carry a nucleotide
  uint64_t xa = 0, xd = 0, xi = 0;
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t p = p0 + j;
    const uint32_t pc = p < len ? p : len - 1u;              // clamped: always a real position
    const uint64_t live = p < lim ? ~0ull : 0ull;
    const uint32_t c = swa_nt(sw, pc);
    xa ^= zob[4u * pc + c] & live;
    xd ^= zob[4u * (pc > 0u ? pc - 1u : 0u) + c] & (pc > 0u ? live : 0ull);
    xi ^= zob[4u * (pc + 1u) + c] & live;
  }
  uint64_t ea = xa, ed = xd, ei = xi;                        // inclusive prefix scans over the lanes
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const uint64_t ta = swa_shfl_up_u64(ea, d);
    const uint64_t td = swa_shfl_up_u64(ed, d);
    const uint64_t ti = swa_shfl_up_u64(ei, d);
    const uint64_t take = lane >= (int)d ? ~0ull : 0ull;
    ea ^= ta & take; ed ^= td & take; ei ^= ti & take;
  }
  uint64_t pa = baseA ^ ea ^ xa;                             // prefix of the a-stream below p0
  uint64_t sd = tailD ^ ed ^ xd;                             // suffix of the d-stream from p0 on
  uint64_t si = tailI ^ ei ^ xi;                             // suffix of the i-stream from p0 on

  uint32_t prevc = (p0 >= 1u && p0 - 1u < len) ? swa_nt(sw, p0 - 1u) : 4u;
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t p = p0 + j;
    const uint32_t pc = p < len ? p : len;                   // clamped row of the Zobrist table (len is valid)
    const uint32_t in_seq = (p < lim) ? 1u : 0u;
    const uint32_t in_ins = (p < pe && p <= len) ? 1u : 0u;
    const uint32_t c = swa_nt(sw, p < len ? p : len - 1u);
    const uint64_t seq_mask = in_seq ? ~0ull : 0ull;
    uint64_t z[4];
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) { z[b] = zob[4u * pc + b]; }
    const uint64_t zc = (c == 0u) ? z[0] : (c == 1u) ? z[1] : (c == 2u) ? z[2] : z[3];
    const uint64_t za = zc & seq_mask;
    const uint64_t zd = zob[4u * (pc > 0u ? pc - 1u : 0u) + c] & (pc > 0u ? seq_mask : 0ull);
    const uint64_t zi = zob[4u * (pc + 1u) + c] & seq_mask;
    const uint32_t first = (p == 0u) ? 1u : 0u;
    SlotsI s;
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
      s.hs[b] = pa ^ z[b] ^ si;
      s.ok[b] = in_ins & (first | (b != prevc ? 1u : 0u));
      s.code[b] = 2u | (b << 2) | (p << 4);
    }
#pragma unroll
    for (uint32_t t = 0; t < 3u; ++t) {
      const uint32_t b = (t < c) ? t : t + 1u;
      s.hs[4 + t] = H ^ za ^ ((t < c) ? z[t] : z[t + 1u]);
      s.ok[4 + t] = in_seq;
      s.code[4 + t] = 0u | (b << 2) | (p << 4);
    }
    s.hs[7] = pa ^ sd ^ zd;
    s.ok[7] = in_seq & (first | (c != prevc ? 1u : 0u));
    s.code[7] = 1u | (p << 4);
    f(s);
    pa ^= za;
    sd ^= zd;
    si ^= zi;
    prevc = c;
  }
}

// one probe of the candidate (hash h, edit code) drawn from the queue: walk the cluster,
// apply the abundance rule, verify exactly (algod1.cc:558-603, variants.cc:118-165).
// SECOND = the fastidious second level (hash_check_attach, algod1.cc:339-371): no self /
// abundance test there.
template <bool SECOND>
__device__ __forceinline__ bool probe_and_verify(const NetArgs & a, const uint64_t * sw, uint32_t slen,
                                                 uint32_t snw, uint32_t seed, uint64_t seed_abundance,
                                                 uint64_t h, uint32_t code, uint32_t & out_amp,
                                                 int window_filter = 0, uint32_t win_word = 0, uint32_t nwin = 1) {
  const uint32_t type = code & 3u;
  const uint32_t base = (code >> 2) & 3u;
  const uint32_t pos = code >> 4;
  const uint32_t vlen = (type == 0u) ? slen : (type == 1u ? slen - 1u : slen + 1u);
  const uint32_t vnw = (vlen + 31u) >> 5;
  uint64_t idx = (h >> 32) & a.tmask;
  for (;;) {
    const swa_slot s = a.table[idx];
    if (s.amp == kEmpty) { return false; }
    if (s.hash == h) {
      const uint32_t amp = s.amp;
      const uint32_t alen = a.seqlen[amp];
      bool allowed;
      if (SECOND) { const uint32_t hlen = a.seqlen[seed]; allowed = min(hlen, alen) < a.fast_min_len || max(hlen, alen) > a.fast_max_len; }
      else { allowed = amp != seed && (a.no_cluster_breaking != 0 || seed_abundance >= a.abundance[amp]); }
      if (allowed && alen == vlen) {
        const uint64_t * y = a.seqs + a.seq_off[amp];
        // window_filter 1: only neighbours that share the seed's prefix-side window, 2: only those that do not
        bool shared = true;                                    // the seed's prefix-side window, in the neighbour
        for (uint32_t w = 0; w < nwin; ++w) { shared = shared && y[win_word + w] == sw[win_word + w]; }
        bool same = window_filter == 0 || (window_filter == 1 ? shared : !shared);
        for (uint32_t w = 0; w < vnw; ++w) {
          same = same && (swa_variant_word(sw, snw, type, pos, base, w) == y[w]);
        }
        if (same) {
          out_amp = amp;
          return true;
        }
      }
    }
    idx = (idx + 1) & a.tmask;
  }
}

// MODE 0: the d=1 network (query = amplicon first+k of the database).
// MODE 1: fastidious second level (query k = the microvariant tasks[k] of a heavy amplicon;
//         every verified light amplicon gets graft_cand = min(heavy id), algod1.cc:244-258).
// MODE 2: the seeds (or halves of seeds) of the fallback list the anchored passes left.
template <bool ZLDS, int MODE>
__global__ __launch_bounds__(kThreads) void k_d1_probe(const NetArgs a) {
  extern __shared__ uint64_t lds[];
  // LDS carve-up (all 8-byte aligned)
  uint64_t * zob_lds = lds;
  uint64_t * pat = lds + (ZLDS ? 4u * a.zlen : 0u);
  uint64_t * wave_base = pat + 1024;
  const uint32_t seed_words = a.maxwords + 2u;               // + zero padding words
  const uint32_t per_wave = seed_words + kQueueCap + kQueueCap / 2;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  uint64_t * sw = wave_base + (size_t)wave * per_wave;       // staged query words
  uint64_t * qh = sw + seed_words;                           // queue: hashes
  uint32_t * qc = reinterpret_cast<uint32_t *>(qh + kQueueCap);   // queue: edit codes

  if (ZLDS) {
    for (uint32_t i = threadIdx.x; i < 4u * a.zlen; i += kThreads) { zob_lds[i] = a.zobrist[i]; }
  }
  for (uint32_t i = threadIdx.x; i < 1024u; i += kThreads) { pat[i] = a.patterns[i]; }
  __syncthreads();
  const uint64_t * zob = ZLDS ? zob_lds : a.zobrist;

  unsigned long long cand_total = 0;                         // MODE 1: graft candidates found by this wave
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  // this wave's private output segment (a single shared edge counter costs one contended
  // returning atomic per query — measured: ~88 atomics/us on one address bound the kernel)
  const uint32_t gwave = blockIdx.x * kWaves + wave;
  uint32_t seg_at = (MODE == 1) ? 0u : a.seg_fill[gwave];

  const uint32_t nwaves = gridDim.x * kWaves;
  const uint32_t nqueries = (MODE == 2) ? *a.fallback_count : a.count;
  for (uint32_t k = blockIdx.x * kWaves + wave; k < nqueries; k += nwaves) {
    uint32_t seed, len, nw;
    uint32_t range = 0;                                      // MODE 2: 0 all positions, 1 p >= 32, 2 p < 32
    uint64_t seed_ab = 0;
    if (MODE == 0 || MODE == 2) {
      if (MODE == 2) { seed = a.fallback[k].seed; range = a.fallback[k].range; }
      else {
        seed = a.first + k;
        if (a.owner_world > 1u && seed % a.owner_world != a.owner_rank) { continue; }   // another rank's seed (wave-uniform)
      }
      len = a.seqlen[seed];
      nw = (len + 31u) >> 5;
      const uint64_t * gs = a.seqs + a.seq_off[seed];
      seed_ab = a.abundance[seed];
      for (uint32_t w = lane; w < nw + 2u; w += 64u) { sw[w] = (w < nw) ? gs[w] : 0ull; }
    } else {
      // materialise the first-level microvariant (generate_variant_sequence, variants.cc:78-115)
      const swa_task t = a.tasks[k];
      seed = t.heavy;
      const uint32_t hlen = a.seqlen[seed];
      const uint32_t hnw = (hlen + 31u) >> 5;
      const uint64_t * gs = a.seqs + a.seq_off[seed];
      const uint32_t type = t.code & 3u;
      len = (type == 0u) ? hlen : (type == 1u ? hlen - 1u : hlen + 1u);
      nw = (len + 31u) >> 5;
      for (uint32_t w = lane; w < nw + 2u; w += 64u) {
        sw[w] = (w < nw) ? swa_variant_word(gs, hnw, type, t.code >> 4, (t.code >> 2) & 3u, w) : 0ull;
      }
    }
    wave_lds_sync();

    uint32_t qn = 0;          // queue fill (wave uniform)
    uint32_t row = 0;         // hits of this query (wave uniform)

    auto drain = [&](uint32_t cnt) {
      bool hit = false;
      uint32_t amp = 0;
      if ((uint32_t)lane < cnt) {
        // MODE 2: a seed's two halves are divided by the prefix-side window itself, as the pair kernels divide them — range 1
        // keeps only neighbours that share it, range 2 only those that do not.  (By position alone the halves overlap: a
        // deletion at position 31, or inside a run that ends there, is listed at a position >= pb AND changes the window.)
        const int wf = MODE != 2 ? 0 : (int)range;
        hit = probe_and_verify<MODE == 1>(a, sw, len, nw, seed, seed_ab, qh[lane], qc[lane], amp, wf, a.win_word, MODE == 2 ? a.anchor_w / 32u : 1u);
      }
      const uint64_t hm = __ballot(hit);
      if (hm != 0ull) {
        const uint32_t nh = (uint32_t)__popcll(hm);
        if (MODE == 0 || MODE == 2) {
          if (hit) {
            const uint64_t at = (uint64_t)seg_at + (uint64_t)__popcll(hm & lane_lt);
            if (at < a.seg_cap) { a.edges[(uint64_t)gwave * a.seg_cap + at] = ((uint64_t)seed << 32) | amp; }
          }
          seg_at += nh;
        } else {
          if (hit) { atomicMin(&a.graft[amp], seed); }
        }
        row += nh;
      }
    };

    auto enqueue = [&](bool pass, uint64_t h, uint32_t code) {
      const uint64_t m = __ballot(pass);
      if (m == 0ull) { return; }
      if (pass) {
        const uint32_t at = qn + (uint32_t)__popcll(m & lane_lt);
        qh[at] = h;
        qc[at] = code;
      }
      qn += (uint32_t)__popcll(m);
      if (qn >= 64u) {
        wave_lds_sync();
        drain(64u);
        const uint32_t rest = qn - 64u;
        uint64_t th = 0;
        uint32_t tc = 0;
        if ((uint32_t)lane < rest) { th = qh[64 + lane]; tc = qc[64 + lane]; }
        __builtin_amdgcn_wave_barrier();
        if ((uint32_t)lane < rest) { qh[lane] = th; qc[lane] = tc; }
        qn = rest;
      }
    };

    // 8 Bloom-word loads in flight per lane, then test + compact
    auto probe_slots = [&](const auto & s) {
      uint64_t word[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        word[i] = s.ok[i] ? a.bloom[(s.hs[i] >> 10) & a.bmask] : ~0ull;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool pass = s.ok[i] && ((word[i] & pat[s.hs[i] & 1023u]) == 0ull);   // bloompat.cc:68-71
        enqueue(pass, s.hs[i], s.code[i]);
      }
    };
    if (MODE == 2) {
      const swa_aux ax = a.aux[seed];
      const bool by_position = a.window_mode == 0u;           // (window mode: every position, the hits are filtered)
      const uint32_t pb = by_position && range == 1u ? ax.pb : 0u;   // range 1 = what the prefix pass would have done (swa_aux::pb)
      const uint32_t pe = by_position && range == 2u ? a.anchor_w : len + 1u;
      const uint32_t erange = by_position ? range : 0u;       // (`range` itself still selects the filter in drain())
      enumerate_range(sw, len, zob, lane, pb, pe < len + 1u ? pe : len + 1u, ax.h, erange == 1u ? ax.a32 : 0ull,
                      erange == 1u ? (ax.dall ^ ax.d32) : ax.dall, erange == 1u ? (ax.iall ^ ax.i32) : ax.iall,
                      probe_slots);
    } else {
      (void)enumerate_variants(sw, len, zob, lane, probe_slots);
    }
    if (qn > 0u) {
      wave_lds_sync();
      drain(qn);
    }
    if (MODE == 1) { cand_total += row; }
    __builtin_amdgcn_wave_barrier();
  }
  if (MODE != 1 && lane == 0) { a.seg_fill[gwave] = seg_at; }
  if (MODE == 1 && lane == 0 && cand_total != 0ull) { atomicAdd(a.cand_counter, cand_total); }
}
