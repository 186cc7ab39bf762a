// mgx_device_memory.hpp -- the one owner of device memory on the host side (mgx_api.cpp, mgx_dg_api.cpp).
// Host only: nothing here is used from device code.
#pragma once

#include "../../include/mgx.h"
#include "mgx_index_tables.hpp"
#include "mgx_internal.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mgx
{
  // allocations held by all arenas of the process (mgx_live_device_allocations)
  inline std::atomic<int64_t> &live_device_allocations()
  {
    static std::atomic<int64_t> count{0};
    return count;
  }

  // Owns every device allocation of one API object -- a member of the object -- or the temporaries of one call -- a
  // local -- and frees them in its destructor, on every path out.  The objects' fields and the views the kernels read
  // (OperatorData, BrickData, FreeSchedule, TransferData) stay raw pointers into memory an arena holds.
  // Never here: buffers from the communicator's alloc_device, caller-supplied exchange buffers, mgx_malloc memory,
  // pinned host memory, streams, events, graphs, communicators.
  // Every operation returns a status through report_error; the message names `owner` (the entry point) and the bytes.
  class DeviceArena
  {
  public:
    explicit DeviceArena(const char *owner)
      : owner_(owner)
    {}
    DeviceArena(const DeviceArena &)            = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena()
    {
      if (drain_ && !held_.empty())
        (void)hipStreamSynchronize(drain_stream_);
      for (void *p : held_)
        free_one(p);
    }

    // a local arena whose buffers work in flight on `s` may still read: the stream is drained before they are freed
    void drain_before_release(hipStream_t s)
    {
      drain_        = true;
      drain_stream_ = s;
    }

    int alloc(void **out, size_t bytes)
    {
      *out               = nullptr;
      const hipError_t e = hipMalloc(out, bytes);
      if (e != hipSuccess)
        return failed("hipMalloc", bytes, e);
      if (*out) // (zero bytes: no allocation)
        {
          held_.push_back(*out);
          ++live_device_allocations();
        }
      return MGX_OK;
    }
    template <typename T>
    int alloc(T **out, size_t count)
    {
      return alloc(reinterpret_cast<void **>(out), sizeof(T) * count);
    }

    // count + extra entries, the first `count` copied from the host
    template <typename T>
    int upload(T **out, const T *host, size_t count, size_t extra = 0)
    {
      const int status = alloc(out, count + extra);
      return status != MGX_OK ? status : copy(*out, host, sizeof(T) * count);
    }
    template <typename T>
    int upload(T **out, const std::vector<T> &host, size_t extra = 0)
    {
      return upload(out, host.data(), host.size(), extra);
    }
    // `bytes` of any object (the structs of 1D tables)
    int upload_bytes(void **out, const void *host, size_t bytes)
    {
      const int status = alloc(out, bytes);
      return status != MGX_OK ? status : copy(*out, host, bytes);
    }

    // host doubles into an existing device array of the number type / into a new one of n + extra entries
    int copy_as(int number, void *dev_dst, const double *host, size_t n)
    {
      if (number == MGX_F64)
        return copy(dev_dst, host, sizeof(double) * n);
      const std::vector<float> tmp(host, host + n);
      return copy(dev_dst, tmp.data(), sizeof(float) * n);
    }
    int upload_as(int number, void **out, const double *host, size_t n, size_t extra = 0)
    {
      const int status = alloc(out, (number == MGX_F64 ? sizeof(double) : sizeof(float)) * (n + extra));
      return status != MGX_OK ? status : copy_as(number, *out, host, n);
    }

    // a new array of zeros, set on stream `s` (not synchronised)
    int zeros(void **out, size_t bytes, hipStream_t s)
    {
      const int status = alloc(out, bytes);
      if (status != MGX_OK || bytes == 0)
        return status;
      const hipError_t e = hipMemsetAsync(*out, 0, bytes, s);
      return e == hipSuccess ? MGX_OK : failed("hipMemsetAsync", bytes, e);
    }
    template <typename T>
    int zeros(T **out, size_t count, hipStream_t s)
    {
      return zeros(reinterpret_cast<void **>(out), sizeof(T) * count, s);
    }

    // frees a buffer that is replaced while its owner lives; the caller's pointer is left as it is.  nullptr: nothing
    // to do.  The caller has made sure that no work in flight reads the buffer.
    void release(void *ptr)
    {
      if (!ptr)
        return;
      const auto it = std::find(held_.begin(), held_.end(), ptr);
      assert(it != held_.end() && "DeviceArena::release: not a buffer of this arena");
      if (it == held_.end())
        return;
      held_.erase(it);
      free_one(ptr);
    }

  private:
    static void free_one(void *p)
    {
      (void)hipFree(p);
      --live_device_allocations();
    }
    int copy(void *dev, const void *host, size_t bytes)
    {
      if (bytes == 0)
        return MGX_OK;
      const hipError_t e = hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice);
      return e == hipSuccess ? MGX_OK : failed("hipMemcpy to the device", bytes, e);
    }
    int failed(const char *what, size_t bytes, hipError_t e) const
    {
      return report_error(MGX_ERR_HIP, std::string(owner_) + ": " + what + " of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    }

    const char         *owner_;
    std::vector<void *> held_;
    bool                drain_        = false;
    hipStream_t         drain_stream_ = nullptr;
  };

  // a colouring of cells (mgx_index_tables.hpp) as the launchers read it: the order on the device, in the arena of the
  // object that holds `out`
  inline int upload_colours(DeviceArena &mem, ColourLists &out, const CellColouring &colours)
  {
    out.n = colours.n;
    std::copy(colours.start, colours.start + 33, out.start);
    return mem.upload(&out.order, colours.order);
  }
} // namespace mgx
