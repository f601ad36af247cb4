// Robust pose-graph optimisation of a batch of fragment graphs (include/d3feat_hip.h: d3f_pose_graph_optimize): ONE
// workgroup per graph carries the whole two-pass Levenberg-Marquardt loop of csrc/posegraph.hpp -- components, incidence
// lists, edge blocks, assembly by owner rows, the blocked Cholesky with its panel in LDS, the substitutions, the trial
// poses and the accept / reject decision -- so a call is one launch with no host synchronisation, no grid barrier, no
// allocation and no floating-point atomic.  The problem is small (a 3DMatch scene has 37-66 fragments), so it is a
// latency problem: the dense [6N, 6N] matrices (1.25 MB at 66 nodes) stay in L2 and only the 6-row panel of the block
// column being factored, the right-hand side and a few scalars live in LDS.
// The host twin runs the same template with a team of one, which is what the CPU tests (and a sanitizer build of this
// file's host side) check the index arithmetic with.
#include "common.hpp"
#include "posegraph.hpp"

namespace {

using namespace d3f::posegraph;

constexpr int kThreads = 512;

struct DeviceTeam {
  d3f::PhaseClock clock;   // armed by d3f_debug_set_phase_clock (profiles/posegraph_bench.py); idle otherwise
  __device__ int tid() const { return (int)threadIdx.x; }
  __device__ int nt() const { return (int)blockDim.x; }
  __device__ void sync() { __syncthreads(); }
  __device__ void lap(int phase) { clock.lap(phase); }
};

struct HostTeam {
  int tid() const { return 0; }
  int nt() const { return 1; }
  void sync() {}
  void lap(int) {}
};

__global__ void __launch_bounds__(kThreads) pose_graph_kernel(Args a, unsigned long long* phase_clock) {
  __shared__ Scratch s;
  DeviceTeam x;
  x.clock.start(phase_clock);
  run_graph(a, (int)blockIdx.x, s, x);
  x.clock.done();
}

size_t graph_bytes(int max_nodes, int max_edges) { return Layout(nullptr, max_nodes, max_edges).bytes; }

// the checks both entries share; D3F_OK with G == 0 means there is nothing to do
int prepare(const int32_t* node_start, const int32_t* edge_start, int G, int N, int E, int max_nodes, int max_edges,
            const double* poses, const int32_t* edges, const double* Z, const double* info, const int32_t* uncertain,
            double max_distance, double preference, double prune_threshold, int max_iters, double step_tol,
            double rel_cost, double* out_poses, double* weight, int32_t* pruned, int32_t* component,
            int32_t* iterations, double* cost, int32_t* status, void* ws, size_t ws_bytes, Args& a) {
  if (G < 0 || G > D3F_PG_MAX_GRAPHS || N < 0 || E < 0 || max_nodes < 0 || max_nodes > D3F_PG_MAX_NODES ||
      max_edges < 0 || max_edges > D3F_PG_MAX_EDGES || max_iters < 0 || max_iters > D3F_PG_MAX_ITERS ||
      !(max_distance > 0.0) || !(max_distance < INFINITY) || !(preference > 0.0) || !(preference < INFINITY) ||
      !(prune_threshold >= 0.0) || !(prune_threshold <= 1.0) || !(step_tol >= 0.0) || !(rel_cost >= 0.0))
    return D3F_EINVAL;
  if (G == 0) return D3F_OK;
  if (!node_start || !edge_start || !iterations || !cost || !status || !ws ||
      (N > 0 && (!poses || !out_poses || !component)) ||
      (E > 0 && (!edges || !Z || !info || !uncertain || !weight || !pruned)))
    return D3F_EINVAL;
  const size_t stride = graph_bytes(max_nodes, max_edges);
  if (ws_bytes < stride * (size_t)G) return D3F_EWORKSPACE;
  a.node_start = node_start;
  a.edge_start = edge_start;
  a.poses_in = poses;
  a.edges = edges;
  a.Z = Z;
  a.info = info;
  a.uncertain = uncertain;
  a.poses = out_poses;
  a.weight = weight;
  a.pruned = pruned;
  a.component = component;
  a.iterations = iterations;
  a.cost = cost;
  a.status = status;
  a.ws = (char*)ws;
  a.ws_stride = stride;
  a.max_distance = max_distance;
  a.preference = preference;
  a.prune_threshold = prune_threshold;
  a.step_tol = step_tol;
  a.rel_cost = rel_cost;
  a.max_iters = max_iters;
  a.max_nodes = max_nodes;
  a.max_edges = max_edges;
  a.N = N;
  a.E = E;
  return D3F_OK;
}

}  // namespace

extern "C" {

size_t d3f_pose_graph_optimize_ws_bytes(int G, int max_nodes, int max_edges) {
  if (G <= 0 || max_nodes < 0 || max_nodes > D3F_PG_MAX_NODES || max_edges < 0 || max_edges > D3F_PG_MAX_EDGES)
    return 0;
  return graph_bytes(max_nodes, max_edges) * (size_t)G;
}

int d3f_pose_graph_optimize(const int32_t* node_start, const int32_t* edge_start, int G, int N, int E, int max_nodes,
                            int max_edges, const double* poses, const int32_t* edges, const double* Z,
                            const double* info, const int32_t* uncertain, double max_distance,
                            double preference_loop_closure, double prune_threshold, int max_iters, double step_tol,
                            double rel_cost, double* out_poses, double* weight, int32_t* pruned, int32_t* component,
                            int32_t* iterations, double* cost, int32_t* status, void* ws, size_t ws_bytes,
                            void* stream) {
  Args a = {};
  const int rc = prepare(node_start, edge_start, G, N, E, max_nodes, max_edges, poses, edges, Z, info, uncertain,
                         max_distance, preference_loop_closure, prune_threshold, max_iters, step_tol, rel_cost,
                         out_poses, weight, pruned, component, iterations, cost, status, ws, ws_bytes, a);
  if (rc != D3F_OK || G == 0) return rc;
  pose_graph_kernel<<<(unsigned)G, kThreads, 0, (hipStream_t)stream>>>(a, d3f::phase_clock_ptr());
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_pose_graph_optimize_host(const int32_t* node_start, const int32_t* edge_start, int G, int N, int E,
                                 int max_nodes, int max_edges, const double* poses, const int32_t* edges,
                                 const double* Z, const double* info, const int32_t* uncertain, double max_distance,
                                 double preference_loop_closure, double prune_threshold, int max_iters,
                                 double step_tol, double rel_cost, double* out_poses, double* weight, int32_t* pruned,
                                 int32_t* component, int32_t* iterations, double* cost, int32_t* status, void* ws,
                                 size_t ws_bytes, void* stream) {
  (void)stream;
  Args a = {};
  const int rc = prepare(node_start, edge_start, G, N, E, max_nodes, max_edges, poses, edges, Z, info, uncertain,
                         max_distance, preference_loop_closure, prune_threshold, max_iters, step_tol, rel_cost,
                         out_poses, weight, pruned, component, iterations, cost, status, ws, ws_bytes, a);
  if (rc != D3F_OK || G == 0) return rc;
  Scratch* s = new Scratch;
  HostTeam x;
  for (int g = 0; g < G; ++g) run_graph(a, g, *s, x);
  delete s;
  return D3F_OK;
}

int d3f_pose_graph_edge_host(const double* Pi_host, const double* Pj_host, const double* Z_host, const double* L_host,
                             double* r_host, double* cost_host, double* Ji_host, double* Jj_host) {
  if (!Pi_host || !Pj_host || !Z_host || !L_host || !r_host || !cost_host || !Ji_host || !Jj_host) return D3F_EINVAL;
  *cost_host = edge_full(Pi_host, Pj_host, Z_host, L_host, r_host, Ji_host, Jj_host);
  return D3F_OK;
}

}  // extern "C"
