// Tuning of the bit-parallel solver: parser and process default (kernels/bitpar/tuning.hpp).
#include "kernels/bitpar/tuning.hpp"

#include <cstdio>
#include <cstdlib>

#include "msbfs/common.hpp"

namespace msbfs {
namespace bp {

namespace {
double to_num(const std::string& key, const std::string& v) {
  char* end = nullptr;
  const double x = strtod(v.c_str(), &end);
  if (v.empty() || !end || *end) fail("tuning: bad value '" + v + "' for " + key);
  return x;
}
}  // namespace

void Tuning::set(const std::string& key, const std::string& v) {
  if (key == "gamma") gamma = to_num(key, v);
  else if (key == "gamma2") {
    gamma2 = to_num(key, v);
    gamma2_auto = false;
  }
  else if (key == "pfx") {
    pfx = (int)to_num(key, v);
    if (pfx != 0 && pfx != 2) fail("tuning: pfx must be 0 (whole rows) or 2 (prefix pull)");
  } else if (key == "codes") codes = (int)to_num(key, v);
  else if (key == "code_deg") code_deg = to_num(key, v);
  else if (key == "lean") lean = (int)to_num(key, v);
  else if (key == "lean_min") lean_min = (int64_t)to_num(key, v);
  else if (key == "lazy") lazy = (int)to_num(key, v);
  else if (key == "td_fused") td_fused = (int)to_num(key, v);
  else if (key == "td_bm") td_bm = (int64_t)to_num(key, v);
  else if (key == "batch") {
    batch = (int)to_num(key, v);
    if (batch < 1 || batch > 64) fail("tuning: batch must be in [1, 64]");
  } else if (key == "bu_max") bu_max = (int64_t)to_num(key, v);
  else if (key == "tiles") tiles = (int)to_num(key, v);
  else if (key == "tiles_code_deg") tiles_code_deg = to_num(key, v);
  else if (key == "full") full = (int)to_num(key, v);
  else if (key == "dskip") dskip = (int)to_num(key, v);
  else if (key == "push_after") push_after = (int)to_num(key, v);
  else if (key == "dskip3") dskip3 = (int)to_num(key, v);
  else if (key == "chunk2") chunk2 = (int)to_num(key, v);
  else if (key == "wide_few") wide_few = (int)to_num(key, v);
  else if (key == "filter_frac") filter_frac = to_num(key, v);
  else if (key == "pfx_h") {
    pfx_h = (int)to_num(key, v);
    if (pfx_h < 0 || pfx_h > 458752) fail("tuning: pfx_h must be in [0, 458752]");
  }
  else if (key == "tiles_w") {
    tiles_w = (int)to_num(key, v);
    if (tiles_w != 4 && tiles_w != 8 && tiles_w != 16) fail("tuning: tiles_w must be 4, 8 or 16");
  }
  else if (key == "leaf") {
    leaf = (int)to_num(key, v);
    if (leaf < -1 || leaf > 1) fail("tuning: leaf must be 0 (off), 1 (on where legal) or -1 (auto)");
  }
  else if (key == "max_grid") {
    const double x = to_num(key, v);  // (range test before the narrowing)
    if (!(x >= 0 && x <= 2048) || x != (double)(int)x)
      fail("tuning: max_grid must be 0 (no cap) or a block count in [1, 2048]");
    max_grid = (int)x;
  }
  else if (key == "dirs") {
    for (char c : v)
      if (c != 'T' && c != 'B' && c != '.') fail("tuning: dirs takes T, B or . per level");
    dirs = v;
  } else {
    fail("tuning: unknown key '" + key +
         "' (gamma gamma2 pfx codes code_deg lean lean_min lazy td_fused td_bm batch bu_max tiles tiles_code_deg full dskip push_after dskip3 chunk2 wide_few pfx_h filter_frac tiles_w leaf max_grid dirs)");
  }
}

void Tuning::parse(const std::string& spec) {
  size_t p = 0;
  while (p < spec.size()) {
    size_t e = spec.find_first_of(",;", p);  // (';' too: shell tools split env lists at ',')
    if (e == std::string::npos) e = spec.size();
    const std::string kv = spec.substr(p, e - p);
    p = e + 1;
    if (kv.empty()) continue;
    const size_t q = kv.find('=');
    if (q == std::string::npos) fail("tuning: expected key=value, got '" + kv + "'");
    set(kv.substr(0, q), kv.substr(q + 1));
  }
}

const Tuning& Tuning::process_default() {
  static const Tuning t = [] {
    Tuning d;
    if (const char* e = getenv("MSBFS_TUNE")) {
      d.parse(e);
      fprintf(stderr, "msbfs: MSBFS_TUNE=%s\n", e);  // never a silent algorithm change
    }
    return d;
  }();
  return t;
}

}  // namespace bp
}  // namespace msbfs
