// The host program of the environment map (tests/test_env_cpu.py builds and runs it; tests/host/walk_host_build.py has the recipe).
// It includes csrc/env.hip unchanged and calls only its __host__ __device__ functions: no HIP call, no launch, no device.
// Usage: env_host DIR.  Every file is raw little-endian, read into a heap buffer of exactly the file's size (an overread lands in a
// redzone of a sanitizer build).  Read:
//   dims.bin    int32 [2]                 E, R
//   box.bin     fp32  [7]                 lo, hi, far
//   env.bin     fp32  [6][E+1][E+1][4]
//   rays.bin    fp32  [R][8]
//   rest.bin    fp32  [R][7]              opacity | rgb_in | g_out of each ray
// Written:
//   rgb.bin     fp32  [R][3]              env_composite_row
//   grad.bin    fp32  [R][9]              env_composite_grad: g_opacity | the gradient of o | d | near | far
//   nodes.bin   fp32  [6 (E+1)^2][8]      env_ray_row of every node
//   owner.bin   int64 [6 (E+1)^2]         env_owner of every node (what upnerf_env_seam copies from)
#include "env.hip"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

namespace {

struct Blob {
  void* p = nullptr;
  size_t n = 0;
};

Blob read_exact(const std::string& path, size_t want) {
  Blob b;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "env_host: cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  b.n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  if (b.n != want) {
    fprintf(stderr, "env_host: %s has %zu bytes, not %zu\n", path.c_str(), b.n, want);
    exit(2);
  }
  if (posix_memalign(&b.p, 64, b.n ? b.n : 1) != 0 || (b.n && fread(b.p, 1, b.n, f) != b.n)) {
    fprintf(stderr, "env_host: cannot read %s\n", path.c_str());
    exit(2);
  }
  fclose(f);
  return b;
}

template <class T>
void write_all(const std::string& path, const std::vector<T>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || fclose(f) != 0) {
    fprintf(stderr, "env_host: cannot write %s\n", path.c_str());
    exit(2);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: env_host DIR\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const Blob dims = read_exact(dir + "dims.bin", 8), bx = read_exact(dir + "box.bin", 28);
  const int E = ((const int32_t*)dims.p)[0], R = ((const int32_t*)dims.p)[1];
  if (!env_size_ok(E) || R < 0) {
    fprintf(stderr, "env_host: bad dims\n");
    return 2;
  }
  const size_t N = (size_t)E + 1, nodes = 6 * N * N;
  const Blob env = read_exact(dir + "env.bin", nodes * 16), rays = read_exact(dir + "rays.bin", (size_t)R * 32);
  const Blob rest = read_exact(dir + "rest.bin", (size_t)R * 28);
  const float* e = (const float*)env.p;
  const float* box = (const float*)bx.p;

  std::vector<float> rgb((size_t)R * 3), grad((size_t)R * 9), rows(nodes * 8);
  std::vector<int64_t> owner(nodes);
  for (int r = 0; r < R; ++r) {
    const float* row = (const float*)rays.p + (size_t)r * 8;
    const float* x = (const float*)rest.p + (size_t)r * 7;
    env_composite_row(e, E, row, x[0], x + 1, &rgb[(size_t)r * 3]);
    env_composite_grad(e, E, row, x[0], x + 4, &grad[(size_t)r * 9], &grad[(size_t)r * 9 + 1]);
  }
  for (size_t n = 0; n < nodes; ++n) {
    env_ray_row(E, (int64_t)n, box, box + 3, box[6], &rows[n * 8]);
    owner[n] = env_owner(E, (int)(n / (N * N)), (int)(n % N), (int)(n / N % N));
  }
  write_all(dir + "rgb.bin", rgb);
  write_all(dir + "grad.bin", grad);
  write_all(dir + "nodes.bin", rows);
  write_all(dir + "owner.bin", owner);
  free(dims.p), free(bx.p), free(env.p), free(rays.p), free(rest.p);
  return 0;
}
