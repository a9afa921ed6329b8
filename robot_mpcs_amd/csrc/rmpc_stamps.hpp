// rmpc_stamps.hpp -- cycle-stamp recorders of the sweeps (SecStamps) and of the fused kernels' pass loops (PassStamps):
// a body under RMPC_STAMPS, none in a production build.  Included by rmpc_sweep.hpp (inside namespace rmpc), behind
// Partials, whose tk words they fill; needs nothing else.

// Development aid (builds with -DRMPC_STAMPS): cycle stamps of the sweeps and of the fused kernels' pass loops.  Like
// RicStamps (rmpc_ric_common.hpp) the recorders have a body in those builds and none otherwise, so the places that
// stamp carry no #ifdef and a production build is the code without them.
enum StampPhase { PH_SWEEP = 0, PH_DEC = 1, PH_RIC = 2, PH_STEP = 3 };   // words 0 .. 3 of a wavefront's record
#ifdef RMPC_STAMPS
// cycles per section of k_sweep / of the arms' sweep call, summed over the wavefronts of all launches
// (static: one copy per translation unit, read through the unit's entries of the variant table)
static __device__ long long g_sst[8];
#endif
// (-DRMPC_STAMPS_CALLS_ONLY beside -DRMPC_STAMPS: the pass loop's stamps alone.  The section stamps stand inside the sweep
//  call and every one of them is a scalar-memory read with its wait: they move what the call's stamp is taken to measure,
//  DESIGN.md 5.1.  The section lines of scripts/fused_stamps.py are empty then.)
#if defined(RMPC_STAMPS) && !defined(RMPC_STAMPS_CALLS_ONLY)
// Sections of a sweep: st(i) adds the cycles since the previous stamp to section i.
struct SecStamps {
  long long acc[8], t0;
  __device__ __forceinline__ void start() {
    for (int i = 0; i < 8; i++) acc[i] = 0;
    t0 = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void operator()(const int i) {
    const long long t = __builtin_amdgcn_s_memtime();
    acc[i] += t - t0;
    t0 = t;
  }
  // sections i0 .. i0 + n - 1 into / out of the tk words of a Partials or a SweepStepOut
  template <class O>
  __device__ __forceinline__ void put(O &o, const int i0, const int n) const {
    for (int i = i0; i < i0 + n; i++) o.tk[i] = acc[i];
  }
  template <class O>
  __device__ __forceinline__ void get(const O &o, const int i0, const int n) {
    for (int i = i0; i < i0 + n; i++) acc[i] = o.tk[i];
  }
  // the first n sections and a call into g_sst (lane0: one lane of the wavefront)
  __device__ __forceinline__ void flush(const bool lane0, const int n) {
    if (lane0) {
      for (int i = 0; i < n; i++) atomicAdd((unsigned long long *)&g_sst[i], (unsigned long long)acc[i]);
      atomicAdd((unsigned long long *)&g_sst[7], 1ull);
    }
  }
};
#else
struct SecStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void operator()(int) {}
  template <class O> __device__ __forceinline__ void put(O &, int, int) const {}
  template <class O> __device__ __forceinline__ void get(const O &, int, int) {}
  __device__ __forceinline__ void flush(bool, int) {}
};
#endif
#ifdef RMPC_STAMPS
// The pass loop of k_fused / k_fused_arm: cycles per phase, event counters and the wavefront's 8-word record in
// FusedWs::stamps (read by scripts/fused_stamps.py and tests/tools/dev_arm_fused_stamps.py).
struct PassStamps {
  long long ph[4], sec[8], hand, t_start, t_a, t_top, t_sub;
  int pass, ipass, nhand, both, nearly;
  __device__ __forceinline__ void start() {
    for (int i = 0; i < 4; i++) ph[i] = 0;
    for (int i = 0; i < 8; i++) sec[i] = 0;
    hand = 0;
    pass = ipass = nhand = both = nearly = 0;
    t_start = t_a = __builtin_amdgcn_s_memtime();
  }
  // hand-over: from the top of a round of the pass loop to the test that ends the round (k_fused: both sites, the top of
  // the pass and the early one behind the decision, round 1); events = epilogues + prologues (their lane 0); early
  // hand-overs = the epilogues of round 1
  __device__ __forceinline__ void hand_begin() { t_top = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void hand_events(const bool left, const bool took, const int round = 0) {
    nhand += __popcll(__ballot(left)) + __popcll(__ballot(took));
    if (round != 0) nearly += __popcll(__ballot(left));
  }
  __device__ __forceinline__ void hand_end() { hand += __builtin_amdgcn_s_memtime() - t_top; }
  // a pass of the wavefront.  inst: lane 0 of every instance that takes the pass; v1: the lane runs the first-pass copy
  // of the sweep call (both copies run when the two halves of k_fused differ).  Round 1 of k_fused (the first sweep behind
  // an early hand-over) belongs to the pass round 0 began: its instance passes count, its cycles go to the same phases.
  __device__ __forceinline__ void pass_begin(const bool inst, const bool v1, const int round = 0) {
    ipass += __popcll(__ballot(inst));
    if (round != 0) return;
    pass++;
    both += (__ballot(v1) != 0ull && __ballot(!v1) != 0ull) ? 1 : 0;
  }
  __device__ __forceinline__ void mark() { t_a = __builtin_amdgcn_s_memtime(); }
  // the cycles since the previous stamp (or mark) belong to phase p
  __device__ __forceinline__ void operator()(const int p) {
    const long long t = __builtin_amdgcn_s_memtime();
    ph[p] += t - t_a;
    t_a = t;
  }
  // k_fused, inside the sweep phase: the sections of the sweep call (lane 0's instance), then [6] unpark + reductions
  // and [7] the ordering point's wait.  (By value: a reference to the caller's partials among the arguments, even of an
  // empty function, changes how production code schedules their initialisation.)
  template <class O>
  __device__ __forceinline__ void sections(const O o) {
#ifndef RMPC_STAMPS_CALLS_ONLY
    for (int i = 0; i < 6; i++) sec[i] += __builtin_amdgcn_readfirstlane((int)o.tk[i]);
#endif
  }
  __device__ __forceinline__ void sweep_returned() { t_sub = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void sweep_reduced() {
    const long long t = __builtin_amdgcn_s_memtime();
    sec[6] += t - t_sub;
    t_sub = t;
  }
  __device__ __forceinline__ void sweep_end() {
    (*this)(PH_SWEEP);
    sec[7] += t_a - t_sub;
  }
  // Record of the wavefront: [0 .. 3] phases, [4] total, [5] passes | passes with both sweep copies << 32 | early
  // hand-overs << 48 (16 bits each for the two counts: a development aid, launches of some hundred passes per wavefront),
  // [7] instance passes | hand-over events << 32.  k_fused (two = true): [6] hand-over cycles, and the sections as a
  // second record at gridDim.x + blockIdx.x; k_fused_arm: [6] the start time.
  __device__ __forceinline__ void store(long long *const stamps, const bool two) {
    if (threadIdx.x == 0) {
      long long *o = stamps + (size_t)blockIdx.x * 8;
      if (two) {
        long long *o2 = stamps + (size_t)(gridDim.x + blockIdx.x) * 8;
        for (int i = 0; i < 8; i++) o2[i] = sec[i];
      }
      for (int i = 0; i < 4; i++) o[i] = ph[i];
      o[4] = __builtin_amdgcn_s_memtime() - t_start;
      o[5] = (long long)pass | ((long long)(both & 0xffff) << 32) | ((long long)(nearly & 0xffff) << 48);
      o[6] = two ? hand : t_start;
      o[7] = (long long)ipass | ((long long)nhand << 32);
    }
  }
};
#else
struct PassStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void hand_begin() {}
  __device__ __forceinline__ void hand_events(bool, bool, int = 0) {}
  __device__ __forceinline__ void hand_end() {}
  __device__ __forceinline__ void pass_begin(bool, bool, int = 0) {}
  __device__ __forceinline__ void mark() {}
  __device__ __forceinline__ void operator()(int) {}
  template <class O> __device__ __forceinline__ void sections(O) {}
  __device__ __forceinline__ void sweep_returned() {}
  __device__ __forceinline__ void sweep_reduced() {}
  __device__ __forceinline__ void sweep_end() {}
  __device__ __forceinline__ void store(long long *, bool) {}
};
#endif
