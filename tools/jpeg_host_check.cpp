// Stand-alone robustness run of the JPEG decoder's host half (csrc/jpeg_host.h) for a host
// sanitizer build; no HIP, no GPU.  For every file of a directory it runs cvl_jpeg::info and
// cvl_jpeg::decode_coefficients on the file itself, on every truncation in steps of 97 bytes and on
// 2000 seeded single-byte corruptions, with the coefficient buffer sized exactly by info (so a
// write past it is a heap overflow the sanitizer reports).  Build and run: tools/README.md.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../cv-lite-object-detection_amd/csrc/jpeg_host.h"

static long g_runs = 0, g_ok = 0, g_unsupported = 0, g_corrupt = 0;

static int run(const uint8_t* d, size_t n) {
  int32_t info[8];
  const int st = cvl_jpeg::info(d, n, info);
  ++g_runs;
  if (st != CVL_OK) {
    uint16_t qt[192];
    int16_t one[64];
    if (cvl_jpeg::decode_coefficients(d, n, one, 64, qt) != st) {
      fprintf(stderr, "info and decode disagree on a refused file\n");
      exit(2);
    }
    (st == CVL_JPEG_UNSUPPORTED ? g_unsupported : g_corrupt)++;
    return st;
  }
  std::vector<int16_t> coef((size_t)info[7]);
  std::vector<uint16_t> qt(192);
  const int ds = cvl_jpeg::decode_coefficients(d, n, coef.data(), coef.size(), qt.data());
  if (ds != CVL_OK && ds != CVL_JPEG_CORRUPT) {
    fprintf(stderr, "unexpected decode status %d\n", ds);
    exit(2);
  }
  (ds == CVL_OK ? g_ok : g_corrupt)++;
  if (coef.size() >= 64 && cvl_jpeg::decode_coefficients(d, n, coef.data(), coef.size() - 64, qt.data()) != CVL_EINVAL) {
    fprintf(stderr, "a short coefficient buffer was accepted\n");
    exit(2);
  }
  return ds;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <directory of test files>\n", argv[0]);
    return 2;
  }
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  std::vector<std::string> names;
  while (dirent* e = readdir(dir))
    if (e->d_name[0] != '.') names.push_back(std::string(argv[1]) + "/" + e->d_name);
  closedir(dir);
  int files = 0, whole_ok = 0;
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  for (const std::string& name : names) {
    FILE* f = fopen(name.c_str(), "rb");
    if (!f) continue;
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + k);
    fclose(f);
    ++files;
    whole_ok += run(data.data(), data.size()) == CVL_OK;
    for (size_t cut = 0; cut < data.size(); cut += 97) {
      // an exact-size copy, so a read past the truncated end is a heap overflow too
      std::vector<uint8_t> part(data.begin(), data.begin() + (long)cut);
      run(part.data(), part.size());
    }
    for (int k = 0; k < 2000 && !data.empty(); ++k) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      const size_t pos = (size_t)((seed >> 24) % data.size());
      const uint8_t old = data[pos];
      data[pos] = (uint8_t)(seed >> 56);
      run(data.data(), data.size());
      data[pos] = old;
    }
  }
  printf("jpeg_host_check: %d files (%d decode whole), %ld runs: %ld ok, %ld unsupported, %ld corrupt\n", files,
         whole_ok, g_runs, g_ok, g_unsupported, g_corrupt);
  return files > 0 ? 0 : 2;
}
