// orbx_lba_math.inc — the local bundle adjustment (include/orbx.h, "local mapping: local bundle adjustment") as phases over
// csrc/orbx_ba_math.inc, shared by orbx_lba_kernel.hip (device) and tests/cpp/lba_ref.cpp (the CPU restatement, g++
// -ffp-contract=off).  A problem is run by LBA_NT lanes.  A phase is a function of the lane number `tid`: it reads what earlier
// phases wrote and writes what belongs to its lane alone (a vertex, an edge list, an owner's rows of the reduced system), so
// the device runs a phase on its 256 lanes between two barriers and the restatement runs it for tid = 0 .. 255 one after the
// other, with the same result.  Who owns what, and therefore the order of every floating-point sum, is fixed HERE, once, as a
// function of the input only; what each side implements on its own is how the lanes' partial sums are folded (a tree over the
// 256 lanes: lane l += lane l + 128, + 64, ... + 1; inside a wave for a free pose's block: lane l += lane l + 32, ... + 1) and the
// sequence of the phases (k_lba; lba_ref.cpp: buildGraph, optimise).  Integer atomics (counts, cursors,
// bit masks, flags) are used where their result does not depend on the order; no floating-point atomic exists.
// The includer defines ORBX_BA_FN, includes orbx_ba_math.inc first, and defines ORBX_LBA_ADD(p, v) (fetch-and-add on an int,
// returns the old value) and ORBX_LBA_OR64(p, v) (on an unsigned long long); with ORBX_LBA_LAYOUT_ONLY only the problem's
// description and its workspace layout are compiled (the host side, which needs neither).
// [from-knowledge] restatements of ORB-SLAM2 / g2o, PARITY UNPINNED.

namespace orbx_lba {
using namespace orbx_ba;

typedef unsigned long long u64;

constexpr int LBA_NT = 256;      // lanes of a problem
constexpr int LBA_MAX_FREE = 64; // ORBX_LBA_MAX_FREE
constexpr int LBA_MAX_N = 6 * LBA_MAX_FREE;
constexpr double LBA_CHI2 = 5.991;
constexpr int LBA_LDS_MAX_FREE = 29;  // free keyframes up to which the reduced system's packed factor fits in LDS beside Shared:
                                      // 8 * 174 * 173 / 2 = 120,408 bytes (30 keyframes: 128,880, past the 160 KiB with Shared)
constexpr int LBA_SCAN = 8;      // vertices whose observer words an owner of the reduced system fetches at a time
// per-vertex arrays [PT_N][mapCap]: the estimate, its backup, Hll (upper triangle), bl, (Hll + lambda I)^-1 (upper triangle), Dinv bl
constexpr int PT_X = 0, PT_XB = 3, PT_HLL = 6, PT_BL = 12, PT_DI = 15, PT_DB = 21, PT_N = 24;
constexpr int ST_BAD = 2, ST_NONFINITE = 4;  // ORBX_LBA_BAD_INPUT, ORBX_LBA_NONFINITE

// One problem: its inputs and its part of the workspace
struct Prob {
  const orbx_keypoint* kps;  // [frames][cap]
  const int32_t* nKps;       // [frames]
  const float* poseIn;       // [frames][12]
  const int32_t* frameOf;    // [nE] the problem's entries: free keyframes first
  const int32_t* rows;       // [nE][cap] mvpMapPoints as indices into the map set
  const float* mapPts;       // [mapCap][3] of the problem's map set
  const uint8_t* mapMask;    // [mapCap] or null
  const float* invSigma2;    // [nLevels]
  int nLevels, cap, mapCap, mapN, nE, nF;
  Cam K;
  double delta;
  // workspace (layout())
  u64 *word, *aword;         // [mapCap] per map point: the free entries that observe it; [mapCap] per vertex: ... through an active edge
  int32_t *cnt, *vertexOf;   // [mapCap] per map point: its edges; its vertex or -1
  int32_t *pidx, *start, *cursor, *pactive;  // per vertex: map point, first edge slot (start[nP] = nEdges), fill cursor, has an active edge
  int32_t *eEnt, *eFeat, *eLvl, *eVert;      // per edge slot: entry, feature, level, vertex
  int32_t* slotOf;           // [nE][cap] (entry, feature) -> edge slot or -1
  float *eU, *eV, *eW;       // per edge slot: measurement, information
  double *eChi2, *eHpl;      // per edge slot: chi2() of the error as last computed; Hpl [18] (free entries)
  double *pt;                // [PT_N][mapCap]
  double *pq, *pR, *pqb;     // [nE][7] q t, [nE][9] rotation matrix, [nF][7] backup
  double* H;                 // the reduced system's strict lower triangle, packed by rows: (i, c) at i (i - 1) / 2 + c (here, or
                             // in LDS when the problem has at most LBA_LDS_MAX_FREE free keyframes: the kernel points it there)
};

template <class T>
ORBX_BA_FN inline T* lbaCarve(size_t* off, uintptr_t base, size_t n) {
  T* p = reinterpret_cast<T*>(base + *off);
  *off += (n * sizeof(T) + 255) / 256 * 256;
  return p;
}
// the workspace of a problem of nE entries (nF free) with `cap` features each and a map set of mapCap points: the arrays in
// order, each 256-byte aligned; returns the bytes (base 0: only counts)
ORBX_BA_FN inline size_t layout(Prob* v, uintptr_t base) {
  size_t off = 0;
  const size_t mc = (size_t)v->mapCap, ec = (size_t)v->nE * (size_t)v->cap, n = 6 * (size_t)v->nF;
  v->word = lbaCarve<u64>(&off, base, mc);
  v->aword = lbaCarve<u64>(&off, base, mc);
  v->cnt = lbaCarve<int32_t>(&off, base, mc);
  v->vertexOf = lbaCarve<int32_t>(&off, base, mc);
  v->pidx = lbaCarve<int32_t>(&off, base, mc);
  v->start = lbaCarve<int32_t>(&off, base, mc + 1);
  v->cursor = lbaCarve<int32_t>(&off, base, mc);
  v->pactive = lbaCarve<int32_t>(&off, base, mc);
  v->eEnt = lbaCarve<int32_t>(&off, base, ec);
  v->eFeat = lbaCarve<int32_t>(&off, base, ec);
  v->eLvl = lbaCarve<int32_t>(&off, base, ec);
  v->eVert = lbaCarve<int32_t>(&off, base, ec);
  v->slotOf = lbaCarve<int32_t>(&off, base, ec);
  v->eU = lbaCarve<float>(&off, base, ec);
  v->eV = lbaCarve<float>(&off, base, ec);
  v->eW = lbaCarve<float>(&off, base, ec);
  v->eChi2 = lbaCarve<double>(&off, base, ec);
  v->eHpl = lbaCarve<double>(&off, base, ec * 18);
  v->pt = lbaCarve<double>(&off, base, mc * PT_N);
  v->pq = lbaCarve<double>(&off, base, (size_t)v->nE * 7);
  v->pR = lbaCarve<double>(&off, base, (size_t)v->nE * 9);
  v->pqb = lbaCarve<double>(&off, base, (size_t)v->nF * 7);
  v->H = lbaCarve<double>(&off, base, n * (n + 1) / 2);
  return off;
}

// the packed factor's bytes for nF free keyframes
ORBX_BA_FN inline size_t factorBytes(int nF) {
  const size_t n = 6 * (size_t)nF;
  return n ? n * (n - 1) / 2 * sizeof(double) : 0;
}

#ifndef ORBX_LBA_LAYOUT_ONLY
// What the lanes of a problem share (LDS on the device)
struct Shared {
  double red[LBA_NT], red2[LBA_NT];
  double Hpp[LBA_MAX_FREE][21], bp[LBA_MAX_FREE][6], maxD[LBA_MAX_FREE];  // by active rank
  double diag[LBA_MAX_N], ldiag[LBA_MAX_N], b[LBA_MAX_N], y[LBA_MAX_N], x[LBA_MAX_N];
  Lm lm;
  Counters cnt;
  u64 activeFree;
  int actEnt[LBA_MAX_FREE], arank[LBA_MAX_FREE];
  int scan[LBA_NT + 1];
  int status, nP, nEdges, nA, n, nActEdges, nActPoints, ok, accepted, more, stop, nLevel1, nErased, bad;
  int iterations[2], trials[2], rejected[2], failures[2], stopReason[2], nActP[2], nActF[2];
  double chi2Initial[2], chi2Final[2], lambda[2];
};

ORBX_BA_FN inline u64 below(int i) { return (1ull << i) - 1ull; }  // i < 64
ORBX_BA_FN inline int popc(u64 v) { return __builtin_popcountll(v); }
ORBX_BA_FN inline void chunkOf(int n, int tid, int* lo, int* hi) {
  const int c = (n + LBA_NT - 1) / LBA_NT;
  const long long a = (long long)tid * c;
  *lo = a < n ? (int)a : n;
  *hi = a + c < n ? (int)(a + c) : n;
}
ORBX_BA_FN inline double* ptAt(const Prob& v, int arr, int j) { return v.pt + (size_t)arr * (size_t)v.mapCap + (size_t)j; }
ORBX_BA_FN inline void ptLoad(const Prob& v, int first, int n, int j, double* out) {
  for (int k = 0; k < n; k++) out[k] = *ptAt(v, first + k, j);
}
ORBX_BA_FN inline void ptStore(const Prob& v, int first, int n, int j, const double* in) {
  for (int k = 0; k < n; k++) *ptAt(v, first + k, j) = in[k];
}
ORBX_BA_FN inline Pose poseOf(const Prob& v, int e) {
  Pose T;
  for (int k = 0; k < 4; k++) T.q[k] = v.pq[(size_t)e * 7 + k];
  for (int k = 0; k < 3; k++) T.t[k] = v.pq[(size_t)e * 7 + 4 + k];
  return T;
}
ORBX_BA_FN inline void poseStore(const Prob& v, int e, const Pose& T) {
  for (int k = 0; k < 4; k++) v.pq[(size_t)e * 7 + k] = T.q[k];
  for (int k = 0; k < 3; k++) v.pq[(size_t)e * 7 + 4 + k] = T.t[k];
  double R[3][3];
  quatToMatrix(T.q, R);
  for (int k = 0; k < 9; k++) v.pR[(size_t)e * 9 + k] = R[k / 3][k % 3];
}
// the strict lower triangle of the reduced system
ORBX_BA_FN inline double* hAt(const Prob& v, int i, int c) { return v.H + ((size_t)i * (size_t)(i - 1) / 2 + (size_t)c); }

// ---- the graph from the rows ------------------------------------------------------------------------------------------------
// the problem's own lists: counts inside capacity, no frame twice, finite poses.  (v.mapN is checked by the caller's lane 0.)
ORBX_BA_FN inline int checkEntries(const Prob& v, int tid) {
  int bits = 0;
  for (int e = tid; e < v.nE; e += LBA_NT) {
    const int f = v.frameOf[e];
    const int n = v.nKps[f];
    if (n < 0 || n > v.cap) bits |= ST_BAD;
    for (int e2 = 0; e2 < e; e2++)
      if (v.frameOf[e2] == f) bits |= ST_BAD;
    for (int c = 0; c < 12; c++)
      if (!isFiniteF(v.poseIn[(size_t)f * 12 + c])) bits |= ST_NONFINITE;
  }
  return bits;
}
ORBX_BA_FN inline void clearGraph(const Prob& v, int tid) {
  for (int m = tid; m < v.mapCap; m += LBA_NT) {
    v.word[m] = 0;
    v.cnt[m] = 0;
  }
  for (size_t k = tid; k < (size_t)v.nE * (size_t)v.cap; k += LBA_NT) v.slotOf[k] = -1;
}
// does feature f of entry e name a usable map point?  -> its index, or -1; garbage sets *bits and is not followed
ORBX_BA_FN inline int rowPoint(const Prob& v, int e, int fr, int f, int* bits) {
  const int r = v.rows[(size_t)e * v.cap + f];
  if (r >= v.mapN) {
    *bits |= ST_BAD;
    return -1;
  }
  if (r < 0 || (v.mapMask && v.mapMask[r] == 0)) return -1;
  const int oct = v.kps[(size_t)fr * v.cap + f].octave;
  if (oct < 0 || oct >= v.nLevels) {
    *bits |= ST_BAD;
    return -1;
  }
  return r;
}
ORBX_BA_FN inline int countEdges(const Prob& v, int tid) {
  int bits = 0;
  for (int e = 0; e < v.nE; e++) {
    const int fr = v.frameOf[e], n = v.nKps[fr];
    for (int f = tid; f < n; f += LBA_NT) {
      const int r = rowPoint(v, e, fr, f, &bits);
      if (r < 0) continue;
      ORBX_LBA_ADD(&v.cnt[r], 1);
      if (e < v.nF) ORBX_LBA_OR64(&v.word[r], 1ull << e);
    }
  }
  return bits;
}
// the vertices: map points with a free observer, ascending; a lane takes a contiguous chunk, lane 0 scans the lanes' counts
ORBX_BA_FN inline void countVertices(const Prob& v, Shared& s, int tid) {
  int lo, hi, c = 0;
  chunkOf(v.mapN, tid, &lo, &hi);
  for (int m = lo; m < hi; m++) c += v.word[m] != 0 ? 1 : 0;
  s.scan[tid] = c;
}
ORBX_BA_FN inline void scanLanes(Shared& s) {  // lane 0
  int run = 0;
  for (int t = 0; t < LBA_NT; t++) {
    const int c = s.scan[t];
    s.scan[t] = run;
    run += c;
  }
  s.scan[LBA_NT] = run;
}
ORBX_BA_FN inline int fillVertices(const Prob& v, Shared& s, int tid) {
  int lo, hi, bits = 0;
  chunkOf(v.mapN, tid, &lo, &hi);
  int j = s.scan[tid];
  for (int m = lo; m < hi; m++) {
    if (v.word[m] == 0) {
      v.vertexOf[m] = -1;
      continue;
    }
    v.pidx[j] = m;
    v.vertexOf[m] = j;
    for (int c = 0; c < 3; c++) {
      const float x = v.mapPts[(size_t)m * 3 + c];
      if (!isFiniteF(x)) bits |= ST_NONFINITE;
      *ptAt(v, PT_X + c, j) = (double)x;
    }
    j++;
  }
  return bits;
}
ORBX_BA_FN inline void countSlots(const Prob& v, Shared& s, int tid) {
  int lo, hi, c = 0;
  chunkOf(s.nP, tid, &lo, &hi);
  for (int j = lo; j < hi; j++) c += v.cnt[v.pidx[j]];
  s.scan[tid] = c;
}
ORBX_BA_FN inline void fillStarts(const Prob& v, Shared& s, int tid) {
  int lo, hi;
  chunkOf(s.nP, tid, &lo, &hi);
  int run = s.scan[tid];
  for (int j = lo; j < hi; j++) {
    v.start[j] = run;
    v.cursor[j] = run;
    run += v.cnt[v.pidx[j]];
  }
  if (tid == 0) v.start[s.nP] = s.scan[LBA_NT];
}
ORBX_BA_FN inline void fillEdges(const Prob& v, int tid) {
  int bits = 0;
  for (int e = 0; e < v.nE; e++) {
    const int fr = v.frameOf[e], n = v.nKps[fr];
    for (int f = tid; f < n; f += LBA_NT) {
      const int r = rowPoint(v, e, fr, f, &bits);
      if (r < 0) continue;
      const int j = v.vertexOf[r];
      if (j < 0) continue;
      const int k = ORBX_LBA_ADD(&v.cursor[j], 1);
      const orbx_keypoint& kp = v.kps[(size_t)fr * v.cap + f];
      v.eEnt[k] = e;
      v.eFeat[k] = f;
      v.eU[k] = kp.x;
      v.eV[k] = kp.y;
      v.eW[k] = v.invSigma2[kp.octave];
    }
  }
}
// a vertex's edges in ascending entry (the free entries first); two edges of one entry are garbage
ORBX_BA_FN inline int sortEdges(const Prob& v, Shared& s, int tid) {
  int bits = 0;
  for (int j = tid; j < s.nP; j += LBA_NT) {
    const int a = v.start[j], b = v.start[j + 1];
    for (int k = a + 1; k < b; k++) {
      const int e = v.eEnt[k], f = v.eFeat[k];
      const float u = v.eU[k], vv = v.eV[k], w = v.eW[k];
      int q = k;
      while (q > a && v.eEnt[q - 1] > e) {
        v.eEnt[q] = v.eEnt[q - 1];
        v.eFeat[q] = v.eFeat[q - 1];
        v.eU[q] = v.eU[q - 1];
        v.eV[q] = v.eV[q - 1];
        v.eW[q] = v.eW[q - 1];
        q--;
      }
      v.eEnt[q] = e;
      v.eFeat[q] = f;
      v.eU[q] = u;
      v.eV[q] = vv;
      v.eW[q] = w;
    }
    for (int k = a; k < b; k++) {
      if (k > a && v.eEnt[k] == v.eEnt[k - 1]) bits |= ST_BAD;
      v.eVert[k] = j;
      v.eLvl[k] = 0;
      v.eChi2[k] = 0.0;
      v.slotOf[(size_t)v.eEnt[k] * v.cap + v.eFeat[k]] = k;
    }
  }
  return bits;
}
ORBX_BA_FN inline void loadPoses(const Prob& v, int tid) {
  for (int e = tid; e < v.nE; e += LBA_NT) {
    Pose T;
    const float* p = v.poseIn + (size_t)v.frameOf[e] * 12;
    poseFromRt(p, p + 9, &T);
    poseStore(v, e, T);
  }
}

// ---- one edge ---------------------------------------------------------------------------------------------------------------
struct EdgeLin {
  double chi2, rho[2], o, r[2], A[2][3], B[2][6];
};
// computeError, chi2(), the robust kernel (none: rho = (chi2, 1)); pc = map(T_e, X)
ORBX_BA_FN inline void edgeEval(const Prob& v, int k, const double X[3], bool robust, double pc[3], double e[2], EdgeLin* L) {
  const int ent = v.eEnt[k];
  const Pose T = poseOf(v, ent);
  poseMap(T, X, pc);
  const double w = (double)v.eW[k];
  edgeError(pc, (double)v.eU[k], (double)v.eV[k], w, v.K, v.delta, e, L->rho);
  L->chi2 = e[0] * (w * e[0]) + e[1] * (w * e[1]);
  if (!robust) {
    L->rho[0] = L->chi2;
    L->rho[1] = 1.0;
  }
}
// ... and linearizeOplus with the weights of constructQuadraticForm
ORBX_BA_FN inline void edgeLinearize(const Prob& v, int k, const double X[3], bool robust, EdgeLin* L) {
  double pc[3], e[2], R[3][3];
  edgeEval(v, k, X, robust, pc, e, L);
  const double* Rp = v.pR + (size_t)v.eEnt[k] * 9;
  for (int i = 0; i < 9; i++) R[i / 3][i % 3] = Rp[i];
  edgeJacobians(pc, R, false, v.K, L->A, L->B);
  const double w = (double)v.eW[k];
  L->r[0] = -(w * e[0]) * L->rho[1];
  L->r[1] = -(w * e[1]) * L->rho[1];
  L->o = L->rho[1] * w;
}

// ---- a round's active set (initializeOptimization(0)) -----------------------------------------------------------------------
ORBX_BA_FN inline void activate(const Prob& v, Shared& s, int tid) {
  u64 mine = 0;
  int edges = 0, points = 0;
  for (int j = tid; j < s.nP; j += LBA_NT) {
    u64 aw = 0;
    int act = 0;
    for (int k = v.start[j]; k < v.start[j + 1]; k++)
      if (v.eLvl[k] == 0) {
        act++;
        if (v.eEnt[k] < v.nF) aw |= 1ull << v.eEnt[k];
      }
    v.aword[j] = aw;
    v.pactive[j] = act > 0 ? 1 : 0;
    mine |= aw;
    edges += act;
    points += act > 0 ? 1 : 0;
  }
  if (mine) ORBX_LBA_OR64(&s.activeFree, mine);
  if (edges) ORBX_LBA_ADD(&s.nActEdges, edges);
  if (points) ORBX_LBA_ADD(&s.nActPoints, points);
}
// lane 0, before activate()
ORBX_BA_FN inline void roundClear(Shared& s) {
  s.activeFree = 0;
  s.nActEdges = 0;
  s.nActPoints = 0;
}
// lane 0, behind activate(): the active free poses in entry order, the Levenberg-Marquardt state of a fresh optimize()
ORBX_BA_FN inline void roundStart(const Prob& v, Shared& s, int round) {
  int a = 0;
  for (int i = 0; i < v.nF; i++) {
    if ((s.activeFree >> i) & 1ull) {
      s.arank[i] = a;
      s.actEnt[a] = i;
      a++;
    } else {
      s.arank[i] = -1;
    }
  }
  s.nA = a;
  s.n = 6 * a;
  s.nActP[round] = s.nActPoints;
  s.nActF[round] = a;
  Lm& m = s.lm;
  m.lambda = 0.0; m.ni = 2.0; m.currentChi = 0.0; m.iniChi = 0.0; m.rho = 0.0;
  m.nBad = 0; m.qmax = 0; m.ok = 0;
  m.iterations = 0; m.lmTrials = 0; m.rejected = 0; m.solverFailures = 0; m.stopReason = 0;
  for (int k = 0; k < 21; k++) m.Hpp[k] = 0.0;
  for (int k = 0; k < 6; k++) m.bp[k] = m.xp[k] = 0.0;  // (lmJudge's own pose terms add nothing: poseScale() below)
}
// the errors of the active edges at the current estimates (a round with no iteration classifies with these); a lane's chi2 sum
ORBX_BA_FN inline double activeErrors(const Prob& v, Shared& s, int tid, bool robust) {
  double chi = 0.0;
  for (int j = tid; j < s.nP; j += LBA_NT) {
    if (!v.pactive[j]) continue;
    double X[3];
    ptLoad(v, PT_X, 3, j, X);
    for (int k = v.start[j]; k < v.start[j + 1]; k++) {
      if (v.eLvl[k] != 0) continue;
      double pc[3], e[2];
      EdgeLin L;
      edgeEval(v, k, X, robust, pc, e, &L);
      v.eChi2[k] = L.chi2;
      chi = chi + L.rho[0];
    }
  }
  return chi;
}

// ---- buildSystem ------------------------------------------------------------------------------------------------------------
// the points' blocks by their owner over the edges in ascending entry: Hll, bl, Hpl of the free edges; the lane's chi2 sum and
// the largest |diagonal entry| of its vertices' Hll
ORBX_BA_FN inline void buildPoints(const Prob& v, Shared& s, int tid, bool robust, double* chi, double* maxd) {
  for (int j = tid; j < s.nP; j += LBA_NT) {
    if (!v.pactive[j]) continue;
    double X[3], Hll[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0};
    ptLoad(v, PT_X, 3, j, X);
    for (int k = v.start[j]; k < v.start[j + 1]; k++) {
      if (v.eLvl[k] != 0) continue;
      EdgeLin L;
      edgeLinearize(v, k, X, robust, &L);
      v.eChi2[k] = L.chi2;
      *chi = *chi + L.rho[0];
      int q = 0;
      for (int r = 0; r < 3; r++) {
        for (int c = r; c < 3; c++, q++) Hll[q] = Hll[q] + (L.A[0][r] * (L.o * L.A[0][c]) + L.A[1][r] * (L.o * L.A[1][c]));
        bl[r] = bl[r] + (L.A[0][r] * L.r[0] + L.A[1][r] * L.r[1]);
      }
      if (v.eEnt[k] < v.nF) {
        double* Hpl = v.eHpl + (size_t)k * 18;
        for (int p = 0; p < 6; p++)
          for (int l = 0; l < 3; l++) Hpl[p * 3 + l] = L.B[0][p] * (L.o * L.A[0][l]) + L.B[1][p] * (L.o * L.A[1][l]);
      }
    }
    ptStore(v, PT_HLL, 6, j, Hll);
    ptStore(v, PT_BL, 3, j, bl);
    for (int q = 0; q < 6; q += (q == 0 ? 3 : 2)) {  // the diagonal: 0, 3, 5
      const double d = Hll[q] < 0.0 ? -Hll[q] : Hll[q];
      if (d > *maxd) *maxd = d;
    }
  }
}
// a free pose's block by one wave: lane l of 64 adds the terms of its features l, l + 64, ... into acc[27] (Hpp's upper
// triangle, then bp); the wave then folds acc (waveFold: lane l += lane l + 32, + 16, ... + 1) and lane 0 keeps the sums
ORBX_BA_FN inline void buildPoseLane(const Prob& v, int ent, int l, bool robust, double acc[27]) {
  for (int k = 0; k < 27; k++) acc[k] = 0.0;
  const int n = v.nKps[v.frameOf[ent]];
  for (int f = l; f < n; f += 64) {
    const int k = v.slotOf[(size_t)ent * v.cap + f];
    if (k < 0 || v.eLvl[k] != 0) continue;
    double X[3];
    ptLoad(v, PT_X, 3, v.eVert[k], X);
    EdgeLin L;
    edgeLinearize(v, k, X, robust, &L);
    int q = 0;
    for (int p = 0; p < 6; p++) {
      for (int c = p; c < 6; c++, q++) acc[q] = acc[q] + (L.B[0][p] * (L.o * L.B[0][c]) + L.B[1][p] * (L.o * L.B[1][c]));
      acc[21 + p] = acc[21 + p] + (L.B[0][p] * L.r[0] + L.B[1][p] * L.r[1]);
    }
  }
}
ORBX_BA_FN inline void buildPoseKeep(Shared& s, int a, const double acc[27]) {  // the wave's lane 0
  double mx = 0.0;
  int q = 0;
  for (int p = 0; p < 6; q += 6 - p, p++) {
    const double d = acc[q] < 0.0 ? -acc[q] : acc[q];
    if (d > mx) mx = d;
  }
  for (int k = 0; k < 21; k++) s.Hpp[a][k] = acc[k];
  for (int k = 0; k < 6; k++) s.bp[a][k] = acc[21 + k];
  s.maxD[a] = mx;
}
// lane 0, behind the build: solve()'s head (optimization_algorithm_levenberg.cpp:61-100)
ORBX_BA_FN inline void iterationStart(Shared& s, int round, int it, double chi, double maxPoint) {
  Lm& m = s.lm;
  m.currentChi = m.iniChi = chi;
  if (it == 0) {
    double mx = maxPoint;
    for (int a = 0; a < s.nA; a++)
      if (s.maxD[a] > mx) mx = s.maxD[a];
    s.chi2Initial[round] = chi;
    m.lambda = 1e-5 * mx;  // computeLambdaInit
    m.ni = 2.0;
    m.nBad = 0;
  }
  m.rho = 0.0;
  m.qmax = 0;
}

// ---- one trial --------------------------------------------------------------------------------------------------------------
// push, setLambda: per vertex (Hll + lambda I)^-1 and Dinv bl
ORBX_BA_FN inline void trialPoints(const Prob& v, Shared& s, int tid) {
  const double lambda = s.lm.lambda;
  for (int j = tid; j < s.nP; j += LBA_NT) {
    if (!v.pactive[j]) continue;
    double X[3], Hll[6], bl[3], Di[3][3], db[3];
    ptLoad(v, PT_X, 3, j, X);
    ptStore(v, PT_XB, 3, j, X);
    ptLoad(v, PT_HLL, 6, j, Hll);
    ptLoad(v, PT_BL, 3, j, bl);
    pointDinv(Hll, lambda, Di);
    for (int l = 0; l < 3; l++) db[l] = (Di[l][0] * bl[0] + Di[l][1] * bl[1]) + Di[l][2] * bl[2];
    const double du[6] = {Di[0][0], Di[0][1], Di[0][2], Di[1][1], Di[1][2], Di[2][2]};
    ptStore(v, PT_DI, 6, j, du);
    ptStore(v, PT_DB, 3, j, db);
  }
}
ORBX_BA_FN inline int slotOfFree(const Prob& v, int j, int ent) {  // the edge of vertex j to the free entry `ent` (its bit is set)
  return v.start[j] + popc(v.word[v.pidx[j]] & below(ent));
}
// The reduced system.  Owner o < 6 * nA (nA + 1) / 2 is (block pair (a, c), a <= c, counted row by row of the upper block
// triangle; row p of the block): it adds row p of Hpl_a Dinv Hpl_c^T over the vertices in ascending order whose active word
// has both bits, and writes Hschur = Hpp + lambda I - sum into the lower triangle (the diagonal into s.diag).  Owners behind
// those, o' < 6 nA, are row o' of bschur = bp - sum Hpl Dinv bl.
ORBX_BA_FN inline void schurOwners(const Prob& v, Shared& s, int tid) {
  const int nA = s.nA, nBlocks = nA * (nA + 1) / 2;
  const double lambda = s.lm.lambda;
  for (int o = tid; o < nBlocks * 6 + s.n; o += LBA_NT) {
    if (o >= nBlocks * 6) {
      const int row = o - nBlocks * 6, a = row / 6, p = row % 6, ent = s.actEnt[a];
      const u64 bit = 1ull << ent;
      double acc = 0.0;
      for (int j0 = 0; j0 < s.nP; j0 += LBA_SCAN) {
        u64 w[LBA_SCAN];
        for (int k = 0; k < LBA_SCAN; k++) w[k] = j0 + k < s.nP ? v.aword[j0 + k] : 0;
        for (int k = 0; k < LBA_SCAN; k++) {
            if (!(w[k] & bit)) continue;
            const int j = j0 + k;
            const double* Hpl = v.eHpl + (size_t)slotOfFree(v, j, ent) * 18;
            double db[3];
            ptLoad(v, PT_DB, 3, j, db);
            acc = acc + ((Hpl[p * 3] * db[0] + Hpl[p * 3 + 1] * db[1]) + Hpl[p * 3 + 2] * db[2]);
          }
        }
        s.b[row] = s.bp[a][p] - acc;
        continue;
      }
      int t = o / 6, a = 0;
      const int p = o % 6;
      while (t >= nA - a) {
        t -= nA - a;
        a++;
      }
      const int c = a + t, entA = s.actEnt[a], entC = s.actEnt[c];
      const u64 both = (1ull << entA) | (1ull << entC);
      double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int j0 = 0; j0 < s.nP; j0 += LBA_SCAN) {  // (the words of LBA_SCAN vertices fetched together: most have not both bits)
        u64 w[LBA_SCAN];
        for (int k = 0; k < LBA_SCAN; k++) w[k] = j0 + k < s.nP ? v.aword[j0 + k] : 0;
        for (int k = 0; k < LBA_SCAN; k++) {
        if ((w[k] & both) != both) continue;
        const int j = j0 + k;
        const double* Ha = v.eHpl + (size_t)slotOfFree(v, j, entA) * 18;
        const double* Hc = v.eHpl + (size_t)slotOfFree(v, j, entC) * 18;
        double du[6], W[3];
        ptLoad(v, PT_DI, 6, j, du);
        const double Di[3][3] = {{du[0], du[1], du[2]}, {du[1], du[3], du[4]}, {du[2], du[4], du[5]}};
        for (int l = 0; l < 3; l++) W[l] = (Ha[p * 3] * Di[0][l] + Ha[p * 3 + 1] * Di[1][l]) + Ha[p * 3 + 2] * Di[2][l];
        for (int q = 0; q < 6; q++) acc[q] = acc[q] + ((W[0] * Hc[q * 3] + W[1] * Hc[q * 3 + 1]) + W[2] * Hc[q * 3 + 2]);
      }
    }
    const int row = 6 * a + p;
    if (a == c) {
      // Hpp's upper triangle, row p: entries (p, q), q >= p, start at p * 6 - p (p - 1) / 2
      const int base = p * 6 - p * (p - 1) / 2;
      for (int q = p; q < 6; q++) {
        double h = s.Hpp[a][base + (q - p)];
        if (q == p) h = h + lambda;
        const double val = h - acc[q];
        if (q == p)
          s.diag[row] = val;
        else
          *hAt(v, 6 * a + q, row) = val;
      }
    } else {
      for (int q = 0; q < 6; q++) *hAt(v, 6 * c + q, row) = 0.0 - acc[q];
    }
  }
}
// The dense unpivoted Cholesky factorisation, column jc: every lane reads the pivot (false: not > 0 or not finite, the solve
// failed); the lanes scale the column below it; then (cholUpdate, behind a barrier) the trailing update, lane (ti, tc) of a
// 16 x 16 arrangement taking the rows jc + 1 + ti, + 16, ... and of each the columns jc + 1 + tc, + 16, ...: every element gets
// its terms in ascending jc.
ORBX_BA_FN inline bool cholColumn(const Prob& v, Shared& s, int jc, int tid) {
  const double d = s.diag[jc];
  if (!(d > 0.0) || !isFinite(d)) return false;
  const double ljj = sqrt(d);
  if (tid == 0) s.ldiag[jc] = ljj;
  for (int i = jc + 1 + tid; i < s.n; i += LBA_NT) *hAt(v, i, jc) = *hAt(v, i, jc) / ljj;
  return true;
}
ORBX_BA_FN inline void cholUpdate(const Prob& v, Shared& s, int jc, int tid) {
  const int ti = tid >> 4, tc = tid & 15;
  for (int i = jc + 1 + ti; i < s.n; i += 16) {
    const double lij = *hAt(v, i, jc);
    for (int c = jc + 1 + tc; c <= i; c += 16) {
      if (c == i)
        s.diag[i] = s.diag[i] - lij * lij;
      else
        *hAt(v, i, c) = *hAt(v, i, c) - lij * *hAt(v, c, jc);
    }
  }
}
// L y = b column by column, then L^T x = y from the last column up: every lane computes the column's value, lane 0 keeps it
ORBX_BA_FN inline void solveForward(const Prob& v, Shared& s, int jc, int tid) {
  const double yj = s.b[jc] / s.ldiag[jc];
  if (tid == 0) s.y[jc] = yj;
  for (int i = jc + 1 + tid; i < s.n; i += LBA_NT) s.b[i] = s.b[i] - *hAt(v, i, jc) * yj;
}
ORBX_BA_FN inline void solveBackward(const Prob& v, Shared& s, int jc, int tid) {
  const double xj = s.y[jc] / s.ldiag[jc];
  if (tid == 0) s.x[jc] = xj;
  for (int i = tid; i < jc; i += LBA_NT) s.y[i] = s.y[i] - *hAt(v, jc, i) * xj;
}
ORBX_BA_FN inline int solutionBad(const Shared& s, int tid) {
  int bad = 0;
  for (int i = tid; i < s.n; i += LBA_NT) bad |= !isFinite(s.x[i]);
  return bad;
}
// update(): the active free poses (lane a < nA: oplus, the backup first) and the active vertices (xl = Dinv (bl - Hpl^T xp)
// over the vertex's free active edges in ascending entry, its part of computeScale into *scale, X += xl; xlOut [nP][3], when
// given, receives the steps)
ORBX_BA_FN inline void trialStep(const Prob& v, Shared& s, int tid, double* scale, double* xlOut = nullptr) {
  if (tid < s.nA) {
    const int ent = s.actEnt[tid];
    for (int k = 0; k < 7; k++) v.pqb[(size_t)ent * 7 + k] = v.pq[(size_t)ent * 7 + k];
    Pose T = poseOf(v, ent);
    if (poseOplus(s.x + 6 * tid, &T)) ORBX_LBA_ADD(&s.cnt.smallTheta, 1);
    poseStore(v, ent, T);
  }
  const double lambda = s.lm.lambda;
  for (int j = tid; j < s.nP; j += LBA_NT) {
    if (!v.pactive[j]) continue;
    double X[3], bl[3], du[6], cl[3], xl[3];
    ptLoad(v, PT_X, 3, j, X);
    ptLoad(v, PT_BL, 3, j, bl);
    ptLoad(v, PT_DI, 6, j, du);
    for (int l = 0; l < 3; l++) cl[l] = bl[l];
    for (int k = v.start[j]; k < v.start[j + 1]; k++) {
      const int ent = v.eEnt[k];
      if (ent >= v.nF) break;  // (the free entries come first)
      if (v.eLvl[k] != 0) continue;
      const double* Hpl = v.eHpl + (size_t)k * 18;
      const double* xp = s.x + 6 * s.arank[ent];
      for (int l = 0; l < 3; l++)
        for (int p = 0; p < 6; p++) cl[l] = cl[l] + Hpl[p * 3 + l] * (-xp[p]);
    }
    const double Di[3][3] = {{du[0], du[1], du[2]}, {du[1], du[3], du[4]}, {du[2], du[4], du[5]}};
    for (int l = 0; l < 3; l++) {
      xl[l] = (Di[l][0] * cl[0] + Di[l][1] * cl[1]) + Di[l][2] * cl[2];
      *scale = *scale + xl[l] * (lambda * xl[l] + bl[l]);
      X[l] = X[l] + xl[l];
      if (xlOut) xlOut[(size_t)j * 3 + l] = xl[l];
    }
    ptStore(v, PT_X, 3, j, X);
  }
}
// computeScale's pose terms in order, then the points' sum (lane 0)
ORBX_BA_FN inline double poseScale(const Shared& s, double scalePoints) {
  double scale = 0.0;
  for (int a = 0; a < s.nA; a++)
    for (int p = 0; p < 6; p++) scale = scale + s.x[6 * a + p] * (s.lm.lambda * s.x[6 * a + p] + s.bp[a][p]);
  return scale + scalePoints;
}
// pop()
ORBX_BA_FN inline void trialRestore(const Prob& v, Shared& s, int tid) {
  if (tid < s.nA) {
    const int ent = s.actEnt[tid];
    Pose T;
    for (int k = 0; k < 4; k++) T.q[k] = v.pqb[(size_t)ent * 7 + k];
    for (int k = 0; k < 3; k++) T.t[k] = v.pqb[(size_t)ent * 7 + 4 + k];
    poseStore(v, ent, T);
  }
  for (int j = tid; j < s.nP; j += LBA_NT) {
    if (!v.pactive[j]) continue;
    double X[3];
    ptLoad(v, PT_XB, 3, j, X);
    ptStore(v, PT_X, 3, j, X);
  }
}
// lane 0: a round's counters
ORBX_BA_FN inline void roundEnd(Shared& s, int round) {
  const Lm& m = s.lm;
  s.iterations[round] = m.iterations;
  s.trials[round] = m.lmTrials;
  s.rejected[round] = m.rejected;
  s.failures[round] = m.solverFailures;
  s.stopReason[round] = m.stopReason;
  s.chi2Final[round] = m.currentChi;
  s.lambda[round] = m.lambda;
}

// ---- the classification behind a round: chi2() of the error as last computed, isDepthPositive at the current estimates ------
ORBX_BA_FN inline int classify(const Prob& v, Shared& s, int tid, uint8_t* outlier) {
  int n = 0;
  for (int k = tid; k < s.nEdges; k += LBA_NT) {
    double X[3], pc[3];
    ptLoad(v, PT_X, 3, v.eVert[k], X);
    poseMap(poseOf(v, v.eEnt[k]), X, pc);
    if (v.eChi2[k] > LBA_CHI2 || !(pc[2] > 0.0)) {
      n++;
      if (outlier)
        outlier[(size_t)v.eEnt[k] * v.cap + v.eFeat[k]] = 1;
      else
        v.eLvl[k] = 1;
    }
  }
  return n;
}
ORBX_BA_FN inline int resultBad(const Prob& v, Shared& s, int tid) {
  int bad = 0;
  for (int j = tid; j < s.nP; j += LBA_NT)
    for (int c = 0; c < 3; c++) bad |= !isFinite(*ptAt(v, PT_X + c, j));
  for (int e = tid; e < v.nF; e += LBA_NT)
    for (int k = 0; k < 7; k++) bad |= !isFinite(v.pq[(size_t)e * 7 + k]);
  if (tid == 0)
    for (int r = 0; r < 2; r++) bad |= !isFinite(s.chi2Initial[r]) || !isFinite(s.chi2Final[r]) || !isFinite(s.lambda[r]);
  return bad;
}
// the outputs of a problem: poseOut / outlier are the problem's own rows; mapOut is the map set's (copied through by the host)
ORBX_BA_FN inline void writeOutputs(const Prob& v, Shared& s, int tid, bool optimised, float* poseOut, float* mapOut) {
  for (int e = tid; e < v.nE; e += LBA_NT) {
    const float* in = v.poseIn + (size_t)v.frameOf[e] * 12;
    float* out = poseOut + (size_t)e * 12;
    if (optimised && e < v.nF) {
      const double* R = v.pR + (size_t)e * 9;
      for (int k = 0; k < 9; k++) out[k] = (float)R[k];
      for (int k = 0; k < 3; k++) out[9 + k] = (float)v.pq[(size_t)e * 7 + 4 + k];
    } else {
      for (int k = 0; k < 12; k++) out[k] = in[k];
    }
  }
  if (optimised)
    for (int j = tid; j < s.nP; j += LBA_NT)
      for (int c = 0; c < 3; c++) mapOut[(size_t)v.pidx[j] * 3 + c] = (float)*ptAt(v, PT_X + c, j);
}
// lane 0.  counted: the graph was built from clean inputs; ran: the rounds ran (a non-finite RESULT keeps its counters)
ORBX_BA_FN inline void writeResult(const Prob& v, const Shared& s, int status, bool counted, bool ran, orbx_lba_result* out) {
  out->status = status;
  out->n_points = counted ? s.nP : 0;
  out->n_edges = counted ? s.nEdges : 0;
  out->n_free = v.nF;
  for (int r = 0; r < 2; r++) {
    out->iterations[r] = ran ? s.iterations[r] : 0;
    out->lm_trials[r] = ran ? s.trials[r] : 0;
    out->rejected_trials[r] = ran ? s.rejected[r] : 0;
    out->solver_failures[r] = ran ? s.failures[r] : 0;
    out->stop_reason[r] = ran ? s.stopReason[r] : 0;
    out->n_active_points[r] = ran ? s.nActP[r] : 0;
    out->n_active_free[r] = ran ? s.nActF[r] : 0;
    const bool num = ran && status == 0;
    out->chi2_initial[r] = num ? s.chi2Initial[r] : 0.0;
    out->chi2_final[r] = num ? s.chi2Final[r] : 0.0;
    out->lambda[r] = num ? s.lambda[r] : 0.0;
  }
  out->n_level1 = ran ? s.nLevel1 : 0;
  out->n_erased = ran && status == 0 ? s.nErased : 0;
}

#endif  // ORBX_LBA_LAYOUT_ONLY

}  // namespace orbx_lba
