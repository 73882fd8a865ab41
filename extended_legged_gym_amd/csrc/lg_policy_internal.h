// lg_policy_internal.h — the host plumbing lg_policy.hip, lg_planner.hip and lg_estimator.hip share beyond the C ABI: the one error channel
// (the thread's message, what lg_mlp_last_error returns), the device preamble and the weight upload of the create functions, and the widths of
// the opaque network handles, to check that the stages of an estimator fit together.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/lgpolicy.h"

// The exported entry point the caller called: the first line of every entry point that can fail is POLICY_ENTRY.  Entry points call each other
// (a collector calls the acts); the outermost name stays, so a message always begins with the call the caller made.
extern thread_local const char* lg_policy_entry;
struct PolicyEntry {
  bool outer;
  explicit PolicyEntry(const char* name) : outer(lg_policy_entry == nullptr) { if (outer) lg_policy_entry = name; }
  ~PolicyEntry() { if (outer) lg_policy_entry = nullptr; }
  PolicyEntry(const PolicyEntry&) = delete; PolicyEntry& operator=(const PolicyEntry&) = delete;
};
#define POLICY_ENTRY PolicyEntry entry_(__func__)

// records "<entry point>: <what>" as the thread's message and returns `status`, so a call site can return it
int lg_policy_fail(int status, const std::string& what);
#define POLICY_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return lg_policy_fail(LG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

// the preamble of a create function: a device exists and `device_id` names one; false + message otherwise.  The caller then opens its DeviceScope.
bool lg_policy_device_ok(int device_id);
// `bytes` of host memory in a fresh device allocation, registered in `allocs` (the owner's destroy frees those); NULL + message on failure
const void* lg_policy_upload(const void* host, size_t bytes, std::vector<void*>& allocs);

// the device a pointer lives on, -1 if it is not device memory: for the calls that take rows and no handle
int lg_policy_device_of(const void* p);

void lg_mlp_widths(const lg_mlp* m, int* layers, int* in, int* out, int* device);
void lg_rnn_widths(const lg_rnn* m, int* type, int* input, int* hidden, int* device);
