// Robust pose-graph optimisation over the fragments of a scene (posegraph.hip; d3f_pose_graph_optimize and its host
// twin d3f_pose_graph_optimize_host): the SE(3) helpers, the edge residual with its Jacobians and weight, and the
// two-pass Levenberg-Marquardt loop of ONE graph.  Everything here is __host__ __device__ and reads no state.  The loop
// is written once for a team of `nt` workers that meet at `sync()`: the kernel runs it with the threads of one workgroup
// (sync = __syncthreads), the host twin with one worker (sync = nothing) -- the same text, so every sum is taken in the
// same order on both sides and the two differ only where the device's sin / cos / atan2 differ from the host's.
//
// Problem (include/d3feat_hip.h states it in full).  Node k: pose P_k (row-major 4x4, rigid; inv() below is the rigid
// inverse [R^T, -R^T t]).  Edge e = (i, j): measurement Z_e mapping fragment j into fragment i, information L_e (6x6,
// moving frame, translation block first), flag `uncertain`.
//   D_e = inv(Z_e) inv(P_i) P_j,   r_e = [D_t ; log(D_R)],   c_e = r_e^T L_e r_e
//   energy = sum over certain edges of c_e + sum over uncertain edges of mu c_e / (mu + c_e)
//   weight l_e = (mu / (mu + c_e))^2 for an uncertain edge, 1 for a certain one
//   update P_k <- P_k Exp(d_k),  Exp([v, w]) = [[R(w), v], [0, 1]],  R(w) the rotation by |w| about w (Rodrigues)
// Jacobians of r_e, exact at every D (M = inv(P_i) P_j = Z D, phi = log(D_R)):
//   d r / d d_j = J_j = [[D_R, 0], [0, Jr^-1(phi)]],  Jr^-1(phi) = I + [phi]x / 2 + C(|phi|) [phi]x^2,
//                 C(a) = (1 - (a/2) cot(a/2)) / a^2   (1/12 + a^2/720 for a < 1e-3)
//   d r / d d_i = J_i = -J_j Ad(inv(M)),  Ad(inv(M)) = [[M_R^T, -M_R^T [M_t]x], [0, M_R^T]]
//
// Levenberg-Marquardt of one pass, f64.  E = energy at the current poses; lambda = kLambda0 at the start of a pass.
//   repeat (one ITERATION = one factorisation attempt; at most max_iters per pass):
//     H = sum l_e J^T L_e J, g = sum l_e J^T L_e r_e with the weights frozen; rows and columns of fixed nodes identity
//     factor H + lambda diag(H) (Cholesky; a pivot that is not > 0 FAILS)
//       failure:  lambda *= 10; beyond kLambdaMax the pass ends with D3F_PG_ST_INDEFINITE
//     d = -(H + lambda diag(H))^-1 g;  trial poses;  E' = their energy
//     E' < E:   accept; lambda = max(lambda / 10, kLambdaMin);
//               the pass ends when max|d| <= step_tol or E - E' <= rel_cost * E
//     else:     reject; the pass ends when max|d| <= step_tol; lambda *= 10; beyond kLambdaMax the pass ends
//   a pass that used max_iters iterations without ending sets D3F_PG_ST_ITER_CAP.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3F_HD __host__ __device__
#else
#define D3F_HD
#endif

namespace d3f {
namespace posegraph {

constexpr int kMaxNodes = 128;            // D3F_PG_MAX_NODES: the LDS panel and vector of the factorisation are sized by it
constexpr int kMaxDim = 6 * kMaxNodes;
constexpr int kEdgeDoubles = 120;         // per edge: l J_i^T L J_i (36), l J_i^T L J_j (36), l J_j^T L J_j (36), l J_i^T L r, l J_j^T L r
constexpr double kLambda0 = 1e-4, kLambdaMin = 1e-12, kLambdaMax = 1e8;
constexpr int kStOk = 0, kStIterCap = 1, kStNonFinite = 2, kStGraph = 4, kStIndefinite = 8;   // D3F_PG_ST_*

// ------------------------------------------------------------------------------------------------ SE(3) helpers
D3F_HD inline bool finite_d(double v) { return v - v == 0.0; }

// c = a^T b (3x3 row-major)
D3F_HD inline void mul_tn3(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) c[3 * r + q] = (a[r] * b[q] + a[3 + r] * b[3 + q]) + a[6 + r] * b[6 + q];
}

// R(w): rotation by |w| about w
D3F_HD inline void so3_exp(const double w[3], double R[9]) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], t = sqrt(t2);
  double A, B;
  if (t < 1e-4) {
    A = 1.0 - t2 / 6.0;
    B = 0.5 - t2 / 24.0;
  } else {
    A = sin(t) / t;
    B = (1.0 - cos(t)) / t2;
  }
  const double x = w[0], y = w[1], z = w[2];
  R[0] = 1.0 - B * (y * y + z * z); R[1] = B * x * y - A * z;         R[2] = B * x * z + A * y;
  R[3] = B * x * y + A * z;         R[4] = 1.0 - B * (x * x + z * z); R[5] = B * y * z - A * x;
  R[6] = B * x * z - A * y;         R[7] = B * y * z + A * x;         R[8] = 1.0 - B * (x * x + y * y);
}

// log(R): the rotation vector of the row-major rotation R, |w| <= pi, through the unit quaternion (w >= 0)
D3F_HD inline void so3_log(const double R[9], double w[3]) {
  const double tr = R[0] + R[4] + R[8];
  double q0, q1, q2, q3;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    q0 = 0.25 * s; q1 = (R[7] - R[5]) / s; q2 = (R[2] - R[6]) / s; q3 = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    q0 = (R[7] - R[5]) / s; q1 = 0.25 * s; q2 = (R[1] + R[3]) / s; q3 = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    q0 = (R[2] - R[6]) / s; q1 = (R[1] + R[3]) / s; q2 = 0.25 * s; q3 = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    q0 = (R[3] - R[1]) / s; q1 = (R[2] + R[6]) / s; q2 = (R[5] + R[7]) / s; q3 = 0.25 * s;
  }
  if (q0 < 0.0) {
    q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3;
  }
  const double sn = sqrt((q1 * q1 + q2 * q2) + q3 * q3);
  const double k = sn < 1e-10 ? 2.0 / q0 : 2.0 * atan2(sn, q0) / sn;
  w[0] = k * q1; w[1] = k * q2; w[2] = k * q3;
}

// Jr^-1(phi) = I + [phi]x / 2 + C [phi]x^2   (row-major 3x3)
D3F_HD inline void so3_right_jacobian_inverse(const double p[3], double J[9]) {
  const double t2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2], t = sqrt(t2);
  double C;
  if (t < 1e-3) {
    C = 1.0 / 12.0 + t2 / 720.0;
  } else {
    const double h = 0.5 * t;
    C = (1.0 - h * cos(h) / sin(h)) / t2;
  }
  const double x = p[0], y = p[1], z = p[2];
  J[0] = 1.0 - C * (y * y + z * z); J[1] = C * x * y - 0.5 * z;       J[2] = C * x * z + 0.5 * y;
  J[3] = C * x * y + 0.5 * z;       J[4] = 1.0 - C * (x * x + z * z); J[5] = C * y * z - 0.5 * x;
  J[6] = C * x * z - 0.5 * y;       J[7] = C * y * z + 0.5 * x;       J[8] = 1.0 - C * (x * x + y * y);
}

// out = P Exp(d), P and out row-major 4x4 (rows 0..2 are written; row 3 is left as it is)
D3F_HD inline void pose_update(const double* P, const double d[6], double* out) {
  double R[9];
  so3_exp(d + 3, R);
  for (int r = 0; r < 3; ++r) {
    const double a = P[4 * r], b = P[4 * r + 1], c = P[4 * r + 2];
    for (int q = 0; q < 3; ++q) out[4 * r + q] = (a * R[q] + b * R[3 + q]) + c * R[6 + q];
    out[4 * r + 3] = ((a * d[0] + b * d[1]) + c * d[2]) + P[4 * r + 3];
  }
}

// ------------------------------------------------------------------------------------------------ one edge
// D = inv(Z) inv(Pi) Pj -> r[6], M_R[9], M_t[3], D_R[9] (what the Jacobians need)
D3F_HD inline void edge_residual(const double* Pi, const double* Pj, const double* Z, double r[6], double MR[9],
                                 double Mt[3], double DR[9]) {
  double Ri[9], Rj[9], Rz[9], dt[3], u[3];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      Ri[3 * a + b] = Pi[4 * a + b];
      Rj[3 * a + b] = Pj[4 * a + b];
      Rz[3 * a + b] = Z[4 * a + b];
    }
    dt[a] = Pj[4 * a + 3] - Pi[4 * a + 3];
  }
  mul_tn3(Ri, Rj, MR);
  for (int a = 0; a < 3; ++a) Mt[a] = (Ri[a] * dt[0] + Ri[3 + a] * dt[1]) + Ri[6 + a] * dt[2];
  mul_tn3(Rz, MR, DR);
  for (int a = 0; a < 3; ++a) u[a] = Mt[a] - Z[4 * a + 3];
  for (int a = 0; a < 3; ++a) r[a] = (Rz[a] * u[0] + Rz[3 + a] * u[1]) + Rz[6 + a] * u[2];
  so3_log(DR, r + 3);
}

// c = r^T L r, rows in order
D3F_HD inline double edge_cost(const double r[6], const double* L) {
  double c = 0.0;
  for (int a = 0; a < 6; ++a) {
    double s = 0.0;
    for (int b = 0; b < 6; ++b) s += L[6 * a + b] * r[b];
    c += r[a] * s;
  }
  return c;
}

D3F_HD inline double edge_weight(double c, double mu, bool uncertain) {
  if (!uncertain) return 1.0;
  const double q = mu / (mu + c);
  return q * q;
}

D3F_HD inline double edge_energy(double c, double mu, bool uncertain) { return uncertain ? mu * c / (mu + c) : c; }

// residual, cost and both Jacobians (row-major 6x6: row = residual component, column = component of d_i / d_j)
D3F_HD inline double edge_full(const double* Pi, const double* Pj, const double* Z, const double* L, double r[6],
                               double Ji[36], double Jj[36]) {
  double MR[9], Mt[3], DR[9], Jr[9], RzT[9], K[9];
  edge_residual(Pi, Pj, Z, r, MR, Mt, DR);
  so3_right_jacobian_inverse(r + 3, Jr);
  for (int a = 0; a < 36; ++a) Ji[a] = Jj[a] = 0.0;
  // D_R M_R^T = Z_R^T;  K = Z_R^T [M_t]x;  Jr M_R^T
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) RzT[3 * a + b] = Z[4 * b + a];
  for (int a = 0; a < 3; ++a) {
    const double x = RzT[3 * a], y = RzT[3 * a + 1], z = RzT[3 * a + 2];
    K[3 * a] = y * Mt[2] - z * Mt[1];
    K[3 * a + 1] = z * Mt[0] - x * Mt[2];
    K[3 * a + 2] = x * Mt[1] - y * Mt[0];
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      Jj[6 * a + b] = DR[3 * a + b];
      Jj[6 * (a + 3) + b + 3] = Jr[3 * a + b];
      Ji[6 * a + b] = -RzT[3 * a + b];
      Ji[6 * a + b + 3] = K[3 * a + b];
      Ji[6 * (a + 3) + b + 3] = -((Jr[3 * a] * MR[3 * b] + Jr[3 * a + 1] * MR[3 * b + 1]) + Jr[3 * a + 2] * MR[3 * b + 2]);
    }
  return edge_cost(r, L);
}

// ------------------------------------------------------------------------------------------------ one graph
struct Args {
  const int32_t* node_start;   // [G+1]
  const int32_t* edge_start;   // [G+1]
  const double* poses_in;      // [N,16]
  const int32_t* edges;        // [E,2], local to the graph
  const double* Z;             // [E,16]
  const double* info;          // [E,36]
  const int32_t* uncertain;    // [E]
  double* poses;               // [N,16]
  double* weight;              // [E]
  int32_t* pruned;             // [E]
  int32_t* component;          // [N]
  int32_t* iterations;         // [G,2]
  double* cost;                // [G,3]
  int32_t* status;             // [G]
  char* ws;
  size_t ws_stride;            // bytes of one graph's workspace
  double max_distance, preference, prune_threshold, step_tol, rel_cost;
  int max_iters, max_nodes, max_edges, N, E;
};

// what the team shares besides the workspace: LDS in the kernel, a local object in the host twin
struct Scratch {
  double panel[6 * kMaxDim];   // the factorisation's block row: panel[6 c + a] = L[c0 + a][c], c < c0
  double vec[kMaxDim];         // right-hand side / step
  double part[64];             // partial sums
  double diag[36];             // the factored diagonal block
  int flag[4];                 // 0: non-finite input, 1: bad edge, 2: factorisation failed, 3: a label changed
};

D3F_HD inline size_t align8(size_t v) { return (v + 7) / 8 * 8; }

// one graph's slice of the workspace for graphs of at most N nodes and E edges
struct Layout {
  double *H, *A, *g, *blocks, *ce, *fe, *ft, *trial;
  int32_t *active, *label, *inc_start, *inc_edge;
  size_t bytes;
  D3F_HD Layout(char* base, int N, int E) {
    const size_t n = 6 * (size_t)N, e = (size_t)E;
    size_t off = 0;
    auto takeD = [&](size_t count) { double* p = (double*)(base + off); off += 8 * count; return p; };
    H = takeD(n * n); A = takeD(n * n); g = takeD(n); blocks = takeD(kEdgeDoubles * e);
    ce = takeD(e); fe = takeD(e); ft = takeD(e); trial = takeD(16 * (size_t)N);
    auto takeI = [&](size_t count) { int32_t* p = (int32_t*)(base + off); off += 4 * count; return p; };
    active = takeI(e); label = takeI(N); inc_start = takeI((size_t)N + 1); inc_edge = takeI(2 * e);
    bytes = (off + 255) / 256 * 256;
  }
};

D3F_HD inline void lower_label(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);          // integer: the fixed point (the component's lowest node) does not depend on the order
#else
  if (v < *p) *p = v;
#endif
}

// x.lap(phase) closes a phase of the measurement clock (posegraph.hip; nothing on the host)
constexpr int kLapSetup = 0, kLapEdges = 1, kLapAssemble = 2, kLapFactor = 3, kLapSolve = 4, kLapTrial = 5;

// sum of v[0..count) in a fixed shape: 64 strided partial sums in index order, then those in order
template <class X>
D3F_HD inline double sum64(const double* v, int count, Scratch& s, X& x) {
  for (int l = x.tid(); l < 64; l += x.nt()) {
    double acc = 0.0;
    for (int e = l; e < count; e += 64) acc += v[e];
    s.part[l] = acc;
  }
  x.sync();
  double total = 0.0;
  for (int l = 0; l < 64; ++l) total += s.part[l];
  x.sync();
  return total;
}

// max |s.vec[0..n)|
template <class X>
D3F_HD inline double absmax64(int n, Scratch& s, X& x) {
  for (int l = x.tid(); l < 64; l += x.nt()) {
    double acc = 0.0;
    for (int e = l; e < n; e += 64) {
      const double a = fabs(s.vec[e]);
      if (!(a <= acc)) acc = a;   // (a non-finite step is rejected by the energy test whatever this returns)
    }
    s.part[l] = acc;
  }
  x.sync();
  double total = 0.0;
  for (int l = 0; l < 64; ++l)
    if (!(s.part[l] <= total)) total = s.part[l];
  x.sync();
  return total;
}

// The view of one graph that the steps below share.
struct Graph {
  int N, E, n;
  const int32_t* edges;
  const double *Z, *info;
  const int32_t* uncertain;
  double* poses;
  Layout w;
  D3F_HD Graph(const Args& a, int g, int n0, int e0, int N_, int E_)
      : N(N_), E(E_), n(6 * N_), edges(a.edges + 2 * (size_t)e0), Z(a.Z + 16 * (size_t)e0),
        info(a.info + 36 * (size_t)e0), uncertain(a.uncertain + e0), poses(a.poses + 16 * (size_t)n0),
        w(a.ws + (size_t)g * a.ws_stride, a.max_nodes, a.max_edges) {}
};

// components over the active edges by min-label propagation; label[k] = lowest node of k's component
template <class X>
D3F_HD inline void label_components(Graph& G, Scratch& s, X& x) {
  for (int k = x.tid(); k < G.N; k += x.nt()) G.w.label[k] = k;
  x.sync();
  for (int round = 0; round < G.N; ++round) {
    if (x.tid() == 0) s.flag[3] = 0;
    x.sync();
    for (int e = x.tid(); e < G.E; e += x.nt()) {
      if (!G.w.active[e]) continue;
      const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
      const int li = G.w.label[i], lj = G.w.label[j];
      if (li != lj) {
        const int m = li < lj ? li : lj;
        lower_label(&G.w.label[i], m);
        lower_label(&G.w.label[j], m);
        s.flag[3] = 1;
      }
    }
    x.sync();
    const int changed = s.flag[3];
    x.sync();
    if (!changed) break;
  }
}

// incidence list of every node over the active edges, in ascending edge order
template <class X>
D3F_HD inline void build_incidence(Graph& G, X& x) {
  for (int k = x.tid(); k < G.N; k += x.nt()) {
    int cnt = 0;
    for (int e = 0; e < G.E; ++e)
      if (G.w.active[e] && (G.edges[2 * e] == k || G.edges[2 * e + 1] == k)) ++cnt;
    G.w.inc_start[k + 1] = cnt;
  }
  x.sync();
  if (x.tid() == 0) {
    G.w.inc_start[0] = 0;
    for (int k = 0; k < G.N; ++k) G.w.inc_start[k + 1] += G.w.inc_start[k];
  }
  x.sync();
  for (int k = x.tid(); k < G.N; k += x.nt()) {
    int pos = G.w.inc_start[k];
    for (int e = 0; e < G.E; ++e)
      if (G.w.active[e] && (G.edges[2 * e] == k || G.edges[2 * e + 1] == k)) G.w.inc_edge[pos++] = e;
  }
  x.sync();
}

// step (a): per active edge at the poses P: cost -> ce, energy term -> fe, the weighted blocks -> blocks
template <class X>
D3F_HD inline void edge_blocks(Graph& G, const double* P, double mu, X& x) {
  for (int e = x.tid(); e < G.E; e += x.nt()) {
    if (!G.w.active[e]) {
      G.w.ce[e] = 0.0;
      G.w.fe[e] = 0.0;
      continue;
    }
    const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
    const double* L = G.info + 36 * (size_t)e;
    double r[6], Ji[36], Jj[36], LJi[36], LJj[36], Lr[6];
    const double c = edge_full(P + 16 * (size_t)i, P + 16 * (size_t)j, G.Z + 16 * (size_t)e, L, r, Ji, Jj);
    const bool unc = G.uncertain[e] != 0;
    const double l = edge_weight(c, mu, unc);
    G.w.ce[e] = c;
    G.w.fe[e] = edge_energy(c, mu, unc);
    for (int a = 0; a < 6; ++a) {
      double sr = 0.0;
      for (int q = 0; q < 6; ++q) sr += L[6 * a + q] * r[q];
      Lr[a] = l * sr;
      for (int b = 0; b < 6; ++b) {
        double si = 0.0, sj = 0.0;
        for (int q = 0; q < 6; ++q) {
          si += L[6 * a + q] * Ji[6 * q + b];
          sj += L[6 * a + q] * Jj[6 * q + b];
        }
        LJi[6 * a + b] = l * si;
        LJj[6 * a + b] = l * sj;
      }
    }
    double* B = G.w.blocks + kEdgeDoubles * (size_t)e;
    for (int a = 0; a < 6; ++a) {
      double gi = 0.0, gj = 0.0;
      for (int q = 0; q < 6; ++q) {
        gi += Ji[6 * q + a] * Lr[q];
        gj += Jj[6 * q + a] * Lr[q];
      }
      B[108 + a] = gi;
      B[114 + a] = gj;
      for (int b = 0; b < 6; ++b) {
        double sii = 0.0, sij = 0.0, sjj = 0.0;
        for (int q = 0; q < 6; ++q) {
          sii += Ji[6 * q + a] * LJi[6 * q + b];
          sij += Ji[6 * q + a] * LJj[6 * q + b];
          sjj += Jj[6 * q + a] * LJj[6 * q + b];
        }
        B[6 * a + b] = sii;
        B[36 + 6 * a + b] = sij;
        B[72 + 6 * a + b] = sjj;
      }
    }
  }
  x.sync();
}

// the energy terms of the active edges at the poses P -> ft
template <class X>
D3F_HD inline void edge_energies(Graph& G, const double* P, double mu, X& x) {
  for (int e = x.tid(); e < G.E; e += x.nt()) {
    double f = 0.0;
    if (G.w.active[e]) {
      const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
      double r[6], MR[9], Mt[3], DR[9];
      edge_residual(P + 16 * (size_t)i, P + 16 * (size_t)j, G.Z + 16 * (size_t)e, r, MR, Mt, DR);
      f = edge_energy(edge_cost(r, G.info + 36 * (size_t)e), mu, G.uncertain[e] != 0);
    }
    G.w.ft[e] = f;
  }
  x.sync();
}

// steps (b), (c): H (entry (r, c), r >= c, at H[c n + r]) and g by node block-row, one owner per matrix row, the
// node's incident edges in ascending order; fixed nodes get identity rows
template <class X>
D3F_HD inline void assemble(Graph& G, X& x) {
  const int n = G.n;
  double* H = G.w.H;
  for (size_t idx = x.tid(); idx < (size_t)n * n; idx += x.nt()) H[idx] = 0.0;
  x.sync();
  for (int c = x.tid(); c < n; c += x.nt()) {
    const int k = c / 6, a = c - 6 * k;
    double* row = H + (size_t)c * n;
    if (G.w.label[k] == k) {
      row[c] = 1.0;
      G.w.g[c] = 0.0;
      continue;
    }
    double gacc = 0.0;
    for (int t = G.w.inc_start[k]; t < G.w.inc_start[k + 1]; ++t) {
      const int e = G.w.inc_edge[t];
      const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
      const double* B = G.w.blocks + kEdgeDoubles * (size_t)e;
      if (i == k) {
        gacc += B[108 + a];
        for (int b = a; b < 6; ++b) row[6 * k + b] += B[6 * a + b];
        if (j > k && G.w.label[j] != j)
          for (int b = 0; b < 6; ++b) row[6 * j + b] += B[36 + 6 * a + b];
      } else {
        gacc += B[114 + a];
        for (int b = a; b < 6; ++b) row[6 * k + b] += B[72 + 6 * a + b];
        if (i > k && G.w.label[i] != i)
          for (int b = 0; b < 6; ++b) row[6 * i + b] += B[36 + 6 * b + a];
      }
    }
    G.w.g[c] = gacc;
  }
  x.sync();
}

// step (d): A = H + lambda diag(H), factored in place by block columns of 6 (left-looking): L[r][c], r >= c, ends at
// A[c n + r] and, mirrored, at A[r n + c] for the back substitution.  Returns false when a pivot is not > 0.
template <class X>
D3F_HD inline bool factor(Graph& G, double lambda, Scratch& s, X& x) {
  const int n = G.n;
  const double* H = G.w.H;
  double* A = G.w.A;
  for (size_t idx = x.tid(); idx < (size_t)n * n; idx += x.nt()) {
    const int c = (int)(idx / n), r = (int)(idx - (size_t)c * n);
    if (r >= c) A[idx] = r == c ? H[idx] + lambda * H[idx] : H[idx];
  }
  if (x.tid() == 0) s.flag[2] = 0;
  x.sync();
  for (int c0 = 0; c0 < n; c0 += 6) {
    for (int idx = x.tid(); idx < 6 * c0; idx += x.nt()) {
      const int c = idx / 6, a = idx - 6 * c;
      s.panel[idx] = A[(size_t)c * n + c0 + a];
    }
    x.sync();
    for (int r = c0 + x.tid(); r < n; r += x.nt()) {
      double acc[6];
      for (int b = 0; b < 6; ++b) acc[b] = c0 + b <= r ? A[(size_t)(c0 + b) * n + r] : 0.0;
      for (int c = 0; c < c0; ++c) {
        const double lr = A[(size_t)c * n + r];
        const double* p = s.panel + 6 * c;
        for (int b = 0; b < 6; ++b) acc[b] -= lr * p[b];
      }
      for (int b = 0; b < 6; ++b)
        if (c0 + b <= r) A[(size_t)(c0 + b) * n + r] = acc[b];
    }
    x.sync();
    if (x.tid() == 0) {
      double* d = s.diag;   // d[6 a + b] = L[c0 + a][c0 + b], b <= a
      bool ok = true;
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b <= a; ++b) d[6 * a + b] = A[(size_t)(c0 + b) * n + c0 + a];
      for (int b = 0; b < 6 && ok; ++b) {
        double piv = d[6 * b + b];
        for (int q = 0; q < b; ++q) piv -= d[6 * b + q] * d[6 * b + q];
        if (!(piv > 0.0) || !finite_d(piv)) {
          ok = false;
          break;
        }
        piv = sqrt(piv);
        d[6 * b + b] = piv;
        for (int a = b + 1; a < 6; ++a) {
          double v = d[6 * a + b];
          for (int q = 0; q < b; ++q) v -= d[6 * a + q] * d[6 * b + q];
          d[6 * a + b] = v / piv;
        }
      }
      if (!ok) s.flag[2] = 1;
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b <= a; ++b) A[(size_t)(c0 + b) * n + c0 + a] = d[6 * a + b];
    }
    x.sync();
    if (s.flag[2]) break;
    for (int r = c0 + 6 + x.tid(); r < n; r += x.nt()) {
      double v[6];
      for (int b = 0; b < 6; ++b) {
        double t = A[(size_t)(c0 + b) * n + r];
        for (int q = 0; q < b; ++q) t -= v[q] * s.diag[6 * b + q];
        v[b] = t / s.diag[6 * b + b];
      }
      for (int b = 0; b < 6; ++b) {
        A[(size_t)(c0 + b) * n + r] = v[b];
        A[(size_t)r * n + c0 + b] = v[b];
      }
    }
    x.sync();
  }
  const bool ok = s.flag[2] == 0;
  x.sync();
  return ok;
}

// s.vec = -(L L^T)^-1 g by forward and back substitution in blocks of 6
template <class X>
D3F_HD inline void solve(Graph& G, Scratch& s, X& x) {
  const int n = G.n;
  const double* A = G.w.A;
  for (int c = x.tid(); c < n; c += x.nt()) s.vec[c] = -G.w.g[c];
  x.sync();
  for (int c0 = 0; c0 < n; c0 += 6) {
    if (x.tid() == 0)
      for (int a = 0; a < 6; ++a) {
        double v = s.vec[c0 + a];
        for (int b = 0; b < a; ++b) v -= A[(size_t)(c0 + b) * n + c0 + a] * s.vec[c0 + b];
        s.vec[c0 + a] = v / A[(size_t)(c0 + a) * n + c0 + a];
      }
    x.sync();
    for (int r = c0 + 6 + x.tid(); r < n; r += x.nt()) {
      double acc = s.vec[r];
      for (int b = 0; b < 6; ++b) acc -= A[(size_t)(c0 + b) * n + r] * s.vec[c0 + b];
      s.vec[r] = acc;
    }
    x.sync();
  }
  for (int c0 = n - 6; c0 >= 0; c0 -= 6) {
    if (x.tid() == 0)
      for (int a = 5; a >= 0; --a) {
        double v = s.vec[c0 + a];
        for (int b = a + 1; b < 6; ++b) v -= A[(size_t)(c0 + a) * n + c0 + b] * s.vec[c0 + b];
        s.vec[c0 + a] = v / A[(size_t)(c0 + a) * n + c0 + a];
      }
    x.sync();
    for (int c = x.tid(); c < c0; c += x.nt()) {
      double acc = s.vec[c];
      for (int b = 0; b < 6; ++b) acc -= A[(size_t)(c0 + b) * n + c] * s.vec[c0 + b];
      s.vec[c] = acc;
    }
    x.sync();
  }
}

// One graph, both passes.  Every worker of the team takes the same branches: what decides them is read from the
// workspace or the scratch after a sync.
template <class X>
D3F_HD inline void run_graph(const Args& a, int g, Scratch& s, X& x) {
  const int tid = x.tid(), nt = x.nt();
  const int n0 = a.node_start[g], n1 = a.node_start[g + 1], e0 = a.edge_start[g], e1 = a.edge_start[g + 1];
  const int N = n1 - n0, E = e1 - e0;
  if (tid == 0) {
    a.iterations[2 * g] = a.iterations[2 * g + 1] = 0;
    a.cost[3 * g] = a.cost[3 * g + 1] = a.cost[3 * g + 2] = 0.0;
  }
  if (n0 < 0 || N < 0 || n1 > a.N || e0 < 0 || E < 0 || e1 > a.E) {   // nothing of this graph can be addressed
    if (tid == 0) a.status[g] = kStGraph;
    return;
  }
  for (int idx = tid; idx < 16 * N; idx += nt) a.poses[16 * (size_t)n0 + idx] = a.poses_in[16 * (size_t)n0 + idx];
  for (int k = tid; k < N; k += nt) a.component[n0 + k] = k;
  for (int e = tid; e < E; e += nt) {
    a.weight[e0 + e] = 0.0;
    a.pruned[e0 + e] = 0;
  }
  if (N > a.max_nodes || E > a.max_edges) {                           // larger than the workspace was sized for
    if (tid == 0) a.status[g] = kStGraph;
    return;
  }
  if (tid == 0) s.flag[0] = s.flag[1] = 0;
  x.sync();
  Graph G(a, g, n0, e0, N, E);
  for (int k = tid; k < N; k += nt) {
    bool ok = true;
    for (int q = 0; q < 12; ++q) ok = ok && finite_d(G.poses[16 * (size_t)k + q]);
    if (!ok) s.flag[0] = 1;
  }
  for (int e = tid; e < E; e += nt) {
    const int i = G.edges[2 * e], j = G.edges[2 * e + 1];
    if (i < 0 || i >= N || j < 0 || j >= N || i == j) s.flag[1] = 1;
    bool zok = true, lok = true;
    for (int q = 0; q < 12; ++q) zok = zok && finite_d(G.Z[16 * (size_t)e + q]);
    for (int q = 0; q < 36; ++q) lok = lok && finite_d(G.info[36 * (size_t)e + q]);
    if (!zok) s.flag[0] = 1;
    const int act = lok && G.info[36 * (size_t)e] > 0.0 ? 1 : 0;
    G.w.active[e] = act;
    if (!act) a.pruned[e0 + e] = 1;
  }
  x.sync();
  const int bad = (s.flag[0] ? kStNonFinite : 0) | (s.flag[1] ? kStGraph : 0);
  x.sync();
  if (bad) {
    if (tid == 0) a.status[g] = bad;
    return;
  }
  int status = kStOk;
  for (int pass = 0; pass < 2; ++pass) {
    label_components(G, s, x);
    build_incidence(G, x);
    // mu = preference * max_distance^2 * mean over the active edges of L[0,0]
    for (int e = tid; e < E; e += nt) {
      G.w.ft[e] = G.w.active[e] ? G.info[36 * (size_t)e] : 0.0;
      G.w.ce[e] = G.w.active[e] ? 1.0 : 0.0;
    }
    x.sync();
    const double sum_n = sum64(G.w.ft, E, s, x), live = sum64(G.w.ce, E, s, x);
    const double mu = live > 0.0 ? a.preference * a.max_distance * a.max_distance * (sum_n / live) : 0.0;
    x.lap(kLapSetup);
    edge_blocks(G, G.poses, mu, x);
    double energy = sum64(G.w.fe, E, s, x);
    x.lap(kLapEdges);
    if (pass == 0 && tid == 0) a.cost[3 * g] = energy;
    double lambda = kLambda0;
    int it = 0;
    bool ended = !(live > 0.0), assembled = false;
    while (!ended && it < a.max_iters) {
      if (!assembled) {
        assemble(G, x);
        assembled = true;
        x.lap(kLapAssemble);
      }
      ++it;
      const bool factored = factor(G, lambda, s, x);
      x.lap(kLapFactor);
      if (!factored) {
        lambda *= 10.0;
        if (lambda > kLambdaMax) {
          status |= kStIndefinite;
          ended = true;
        }
        continue;
      }
      solve(G, s, x);
      x.lap(kLapSolve);
      const double maxd = absmax64(G.n, s, x);
      for (int k = tid; k < N; k += nt) {
        const double* P = G.poses + 16 * (size_t)k;
        double* Q = G.w.trial + 16 * (size_t)k;
        for (int q = 0; q < 16; ++q) Q[q] = P[q];
        if (G.w.label[k] != k) pose_update(P, s.vec + 6 * k, Q);
      }
      x.sync();
      edge_energies(G, G.w.trial, mu, x);
      const double trial_energy = sum64(G.w.ft, E, s, x);
      x.lap(kLapTrial);
      if (trial_energy < energy) {
        for (int idx = tid; idx < 16 * N; idx += nt) G.poses[idx] = G.w.trial[idx];
        x.sync();
        edge_blocks(G, G.poses, mu, x);
        x.lap(kLapEdges);
        assembled = false;
        const double drop = energy - trial_energy;
        if (maxd <= a.step_tol || drop <= a.rel_cost * energy) ended = true;
        energy = trial_energy;
        lambda = lambda / 10.0 > kLambdaMin ? lambda / 10.0 : kLambdaMin;
      } else {
        if (maxd <= a.step_tol) ended = true;
        lambda *= 10.0;
        if (lambda > kLambdaMax) ended = true;
      }
    }
    if (!ended) status |= kStIterCap;
    // the weights at the end of the pass; after the first, the edges the line process switched off leave
    for (int e = tid; e < E; e += nt)
      if (G.w.active[e]) {
        const double l = edge_weight(G.w.ce[e], mu, G.uncertain[e] != 0);
        a.weight[e0 + e] = l;
        if (pass == 0 && G.uncertain[e] != 0 && l < a.prune_threshold) {
          G.w.active[e] = 0;
          a.pruned[e0 + e] = 1;
        }
      }
    if (tid == 0) {
      a.iterations[2 * g + pass] = it;
      a.cost[3 * g + 1 + pass] = energy;
    }
    x.sync();
  }
  for (int k = tid; k < N; k += nt) a.component[n0 + k] = G.w.label[k];
  if (tid == 0) a.status[g] = status;
  x.lap(kLapSetup);
}

}  // namespace posegraph
}  // namespace d3f
