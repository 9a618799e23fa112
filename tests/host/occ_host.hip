// The host program of the occupancy walk (tests/test_walks_host_cpu.py builds and runs it; tests/host/walk_host_build.py has the recipe).
// It includes csrc/occupancy.hip unchanged and calls occ_walk on every ray row: no HIP call, no launch, no device.
// Usage: occ_host DIR.  Raw little-endian files, each read into a heap buffer of exactly its size:
//   dims.bin  int32 [4]  Cx, Cy, Cz, R      bounds.bin  fp32 [6]  lo[3], hi[3]
//   words.bin uint32 [upnerf_occ_words(Cx, Cy, Cz)]      rays.bin  fp32 [R][8]
// Written: t0.bin, t1.bin fp32 [R]; hit.bin uint8 [R].
#include "occupancy.hip"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

namespace {

void* read_exact(const std::string& path, size_t want) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "occ_host: cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc(n ? n : 1);
  if (n != want || !p || (n && fread(p, 1, n, f) != n)) {
    fprintf(stderr, "occ_host: %s has %zu bytes, not %zu, or cannot be read\n", path.c_str(), n, want);
    exit(2);
  }
  fclose(f);
  return p;
}

void write_all(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, 1, n, f) != n) || fclose(f) != 0) {
    fprintf(stderr, "occ_host: cannot write %s\n", path.c_str());
    exit(2);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: occ_host DIR\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  int32_t* dv = (int32_t*)read_exact(dir + "dims.bin", 4 * 4);
  float* bv = (float*)read_exact(dir + "bounds.bin", 6 * 4);
  OccDims dm;
  const int R = dv[3];
  if (!occ_dims(dv[0], dv[1], dv[2], &dm) || R <= 0) {
    fprintf(stderr, "occ_host: bad dims\n");
    return 2;
  }
  const long long n_words = upnerf_occ_words(dv[0], dv[1], dv[2]);
  uint32_t* words = (uint32_t*)read_exact(dir + "words.bin", (size_t)n_words * 4);
  float* rays = (float*)read_exact(dir + "rays.bin", (size_t)R * 32);
  upnerf_occ_spans_args a = {};
  a.Cx = dv[0], a.Cy = dv[1], a.Cz = dv[2], a.R = R;
  for (int k = 0; k < 3; ++k) a.lo[k] = bv[k], a.hi[k] = bv[3 + k];
  a.words = words, a.rays = rays;
  std::vector<float> t0(R), t1(R);
  std::vector<uint8_t> hit(R);
  for (int r = 0; r < R; ++r) hit[r] = occ_walk(a, dm, rays + (size_t)r * 8, &t0[r], &t1[r]) ? 1 : 0;
  write_all(dir + "t0.bin", t0.data(), t0.size() * 4);
  write_all(dir + "t1.bin", t1.data(), t1.size() * 4);
  write_all(dir + "hit.bin", hit.data(), hit.size());
  free(dv), free(bv), free(words), free(rays);
  return 0;
}
