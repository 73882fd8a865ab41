// lg_switches.h — the environment switches of the C++ library (host code only): one table, and the readers that check them.  Every switch is an A/B or
// test hook and the defaults are what ships.  A value outside the accepted set makes the call that reads it fail with LG_ERR_INVALID, the error naming the
// variable and the value.  No other file in csrc/ calls getenv.  INTEGRATION.md ("Environment switches") mirrors the table.
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <string>

struct LgSwitch { const char* name; const char* accepted; const char* deflt; const char* read_at; const char* changes; };
static const LgSwitch lg_switch_table[] = {
  {"LG_FUSE",         "0 | 1",                     "1",    "lg_create",        "0: every step is the physics launch plus post_kernel (no fused tail)"},
  {"LG_SPLIT",        "0 | 1",                     "1",    "lg_create",        "0: no helper waves on height grids and planes (single-wave physics instances)"},
  {"LG_PERSIST",      "0 | 1",                     "1",    "lg_create",        "0: lg_rollout_batch runs one launch per rollout step instead of one per horizon"},
  {"LG_GFUSE",        "0 | 1",                     "0",    "lg_create",        "1: the six-legged lg_step ends inside the physics launch (generic fused tail)"},
  {"LG_CAPS",         "0 | 1",                     "1",    "lg_create",        "0: no capsule segments: every sphere stays in the middle of its part"},
  {"LG_MESH_CAPS",    "0 | 1",                     "1",    "lg_create",        "0: spheres alone on grid meshes (no segments against the mesh's edges)"},
  {"LG_GRID_MESH",    "0 | 1",                     "1",    "lg_create",        "0: grid meshes walk the BVH instead of indexing their cells"},
  {"LG_LATTICE_CAPS", "0 | 1",                     "unset", "lg_create",       "capsule segments on lattice meshes; overrides lg_set_lattice_capsules"},
  {"LG_LATTICE_CAP",  "1 .. 1664",                 "1664", "lg_create",        "entries of a wave's lattice query table; never below the mesh's longest run of faces"},
  {"LG_DEAL",         "0 | permutation of 0-7",    "model", "lg_create",       "contact slot at each wave position on height grids; 0: the identity"},
  {"LG_MESH_DEAL",    "0 | permutation of 0-7",    "model", "lg_create",       "contact slot at each wave position on triangle meshes; 0: model order"},
  {"LG_MESH_REACH",   "0 .. 1 (m)",                "0.05", "lg_create",        "how far ahead the mesh contact distance cache looks"},
  {"LG_CHAIN_EPB",    "1 .. 32",                   "auto", "physics launch",   "envs per workgroup of the two-legged (six joints per leg) physics kernel"},
  {"LG_RAY_GRID",     "0 | 1",                     "1",    "lg_mesh_create",   "0: no ray lattice: rays (and contact queries) walk the BVH"},
  {"LG_LATTICE_CP",   "0 | 1",                     "1",    "lg_mesh_create",   "0: no closest-point cell table: contact queries walk the BVH"},
  {"LG_SDF_LATTICE",  "0 | 1",                     "1",    "every SDF query",  "0: lg_sdf_bodies_update walks the BVH instead of the cell table"},
  {"LG_SDF_ORDER",    "0 | 1",                     "1",    "every SDF query",  "0: one env's bodies side by side in a workgroup instead of one body of several envs"},
  {"LG_SDF_BLOCK",    "64 | 128 | 256",            "128",  "every SDF query",  "threads per workgroup of sdf_bodies_kernel"},
  {"LG_RAY_SKIP",     "0 | 1 | 2 | 9",             "1",    "every depth render", "0: rays walk from the camera; 2: also the coarse walk over blocks; 9: timing probe, every ray misses"},
  {"LG_RNN_FORCE_WIDE", "0 | 1",                   "0",    "lg_rnn_create_wide", "1: a memory of 512 inputs or fewer takes the wide kernels too (projection + seeded step): a test hook for their bits"},
};

static inline bool lg_switch_refuse(const char* name, const char* value, std::string& err) {
  const char* accepted = "?";
  for (const LgSwitch& s : lg_switch_table) if (strcmp(s.name, name) == 0) accepted = s.accepted;
  err = std::string(name) + "=" + value + ": not an accepted value (" + accepted + ")";
  return false;
}
// The readers leave `v` as it is when the switch is unset; for a value outside the accepted set they set `err` and return false.
// an integer in [lo, hi] (decimal digits, nothing else)
static inline bool lg_switch_int(const char* name, int lo, int hi, int& v, std::string& err) {
  const char* s = getenv(name);
  char* end = nullptr;
  const long x = s ? strtol(s, &end, 10) : 0;
  if (s && (!*s || *end || x < lo || x > hi)) return lg_switch_refuse(name, s, err);
  if (s) v = (int)x;
  return true;
}
static inline bool lg_switch_flag(const char* name, int& v, std::string& err) { return lg_switch_int(name, 0, 1, v, err); }
// an integer out of a short list
static inline bool lg_switch_int_in(const char* name, std::initializer_list<int> ok, int& v, std::string& err) {
  int x = v;
  if (!lg_switch_int(name, INT_MIN, INT_MAX, x, err)) return false;
  for (int o : ok) if (o == x) { v = x; return true; }
  return lg_switch_refuse(name, getenv(name), err);
}
static inline bool lg_switch_float(const char* name, float lo, float hi, float& v, std::string& err) {
  const char* s = getenv(name);
  char* end = nullptr;
  const float x = s ? strtof(s, &end) : 0.f;
  if (s && (!*s || *end || !(x >= lo && x <= hi))) return lg_switch_refuse(name, s, err);
  if (s) v = x;
  return true;
}
// "0" = the identity 0x76543210; eight digits that are a permutation of 0..7 = the slots at positions 0..7, four bits each
static inline bool lg_switch_perm8(const char* name, unsigned& v, std::string& err) {
  const char* s = getenv(name);
  if (!s) return true;
  unsigned perm = 0u, seen = 0u;
  for (int p = 0; p < 8 && strlen(s) == 8; ++p) { const unsigned d = (unsigned)(s[p] - '0'); seen |= d < 8u ? 1u << d : 0u; perm |= d << (4 * p); }
  if (strcmp(s, "0") == 0) perm = 0x76543210u;
  else if (seen != 0xffu) return lg_switch_refuse(name, s, err);
  v = perm;
  return true;
}
