// lockstep_solver.h — CG over the ranks of an example through the C ABI (pdh_dcg_*, include/polydeal_hip.h): the ranks are contexts of
// this one process and take every step together, which is what a transport between real ranks does for them.  A halo move is one
// device-to-device copy per pair of ranks, the all-reduce adds the ranks' sums in rank order on the host.  The reference solves on its
// MPI ranks (examples/diffusion_reaction.cc:699-735).
//
// The examples are plain C++ (no HIP headers): the three runtime calls needed for the vectors are looked up in the HIP runtime that
// libpolydeal_hip.so has brought into the process.
#pragma once
#include "../include/polydeal_hip.h"

#include <dlfcn.h>

#include <cstdio>
#include <numeric>
#include <vector>

namespace example_solver
{
struct DeviceMemory
{
  int (*malloc_)(void **, size_t) = nullptr;
  int (*memcpy_)(void *, const void *, size_t, int) = nullptr; // kind: 1 host to device, 2 device to host, 3 device to device
  int (*free_)(void *) = nullptr;
  std::vector<void *> bufs;
  DeviceMemory()
  {
    malloc_ = reinterpret_cast<decltype(malloc_)>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    memcpy_ = reinterpret_cast<decltype(memcpy_)>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    free_ = reinterpret_cast<decltype(free_)>(dlsym(RTLD_DEFAULT, "hipFree"));
  }
  ~DeviceMemory()
  {
    for (void *p : bufs)
      free_(p);
  }
  bool ok() const { return malloc_ && memcpy_ && free_; }
  double *put(const double *h, size_t n)
  {
    void *d = nullptr;
    if (malloc_(&d, (n ? n : 1) * sizeof(double)) != 0)
      return nullptr;
    bufs.push_back(d);
    if (n && memcpy_(d, h, n * sizeof(double), 1) != 0)
      return nullptr;
    return static_cast<double *>(d);
  }
};

// ctx[r]: the context of rank r (rows splits[r] .. splits[r + 1]) with its values assembled and its preconditioner set up.  b and x
// are global vectors on the host, x the initial guess and the solution.  Returns the iteration count, < 0 on error (message printed).
inline int solve_cg_lockstep(const std::vector<pdh_ctx *> &ctx, const std::vector<int> &splits, const std::vector<double> &b, std::vector<double> &x,
                             double rel_tol = 1e-13, int max_iter = 20000)
{
  const int W = (int)ctx.size();
  DeviceMemory mem;
  if (!mem.ok())
    return std::fprintf(stderr, "the HIP runtime is not loaded\n"), -1;
  auto fail = [&](int r) { return std::fprintf(stderr, "rank %d: %s\n", r, pdh_last_error(ctx[r])), -1; };
  std::vector<std::vector<int64_t>> send((size_t)W, std::vector<int64_t>((size_t)W)), recv = send, send_at = send, recv_at = send;
  std::vector<double *> d_b((size_t)W), d_x((size_t)W);
  std::vector<pdh_dcg_request> req((size_t)W);
  const pdh_cg_control control{max_iter, rel_tol, 0.0};
  for (int r = 0; r < W; ++r)
    {
      pdh_halo_info info;
      if (pdh_halo_setup(ctx[r], W, splits.data(), send[r].data(), recv[r].data(), &info) != PDH_OK)
        return fail(r);
      std::exclusive_scan(send[r].begin(), send[r].end(), send_at[r].begin(), (int64_t)0);
      std::exclusive_scan(recv[r].begin(), recv[r].end(), recv_at[r].begin(), (int64_t)0);
      d_b[r] = mem.put(b.data() + splits[r], (size_t)(splits[r + 1] - splits[r]));
      d_x[r] = mem.put(x.data() + splits[r], (size_t)(splits[r + 1] - splits[r]));
      if (!d_b[r] || !d_x[r])
        return std::fprintf(stderr, "rank %d: out of device memory\n", r), -1;
    }
  for (int r = 0; r < W; ++r)
    if (pdh_dcg_begin(ctx[r], &control, d_b[r], d_x[r], &req[r]) != PDH_OK)
      return fail(r);
  pdh_cg_result result{};
  for (;;)
    {
      const int kind = req[0].kind; // (every rank asks for the same thing)
      if (kind == PDH_DCG_DONE)
        break;
      if (kind == PDH_DCG_HALO_BEGIN)
        {
          for (int r = 0; r < W; ++r)
            if (pdh_synchronize(ctx[r]) != PDH_OK)
              return fail(r);
          for (int s = 0; s < W; ++s)
            for (int d = 0; d < W; ++d)
              if (send[s][d] && mem.memcpy_(req[d].d_recv + recv_at[d][s], req[s].d_send + send_at[s][d], (size_t)send[s][d] * sizeof(double), 3) != 0)
                return std::fprintf(stderr, "halo copy %d -> %d failed\n", s, d), -1;
        }
      else if (kind == PDH_DCG_ALLREDUCE)
        {
          double total[3] = {0.0, 0.0, 0.0}, part[3];
          const int m = req[0].n_scalars;
          for (int r = 0; r < W; ++r)
            {
              if (pdh_synchronize(ctx[r]) != PDH_OK || mem.memcpy_(part, req[r].d_scalars, (size_t)m * sizeof(double), 2) != 0)
                return fail(r);
              for (int k = 0; k < m; ++k)
                total[k] = r == 0 ? part[k] : total[k] + part[k];
            }
          for (int r = 0; r < W; ++r)
            if (mem.memcpy_(req[r].d_scalars, total, (size_t)m * sizeof(double), 1) != 0)
              return fail(r);
        }
      for (int r = 0; r < W; ++r)
        if (pdh_dcg_resume(ctx[r], &req[r], &result) != PDH_OK)
          return fail(r);
    }
  for (int r = 0; r < W; ++r)
    if (pdh_synchronize(ctx[r]) != PDH_OK ||
        mem.memcpy_(x.data() + splits[r], d_x[r], (size_t)(splits[r + 1] - splits[r]) * sizeof(double), 2) != 0)
      return fail(r);
  return result.iterations;
}
} // namespace example_solver
