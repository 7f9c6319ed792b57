// Runs the host model build (csrc/model_host.h) alone, without HIP or Python, so that it can run under the
// host compiler's sanitizers (tests/test_model_host.py):
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o model_host_check model_host_check.cpp
//   model_host_check DESC_FILE...
// Each file holds the raw bytes of one mjlModelDesc. One line per file:
//   <file>\trc=<code>\tnefc_max=<n>\tncon_max=<n>\tsizeof_ModelF=<bytes>\tmsg=<text>
#include <cstdio>
#include <memory>
#include <string>

#include "../mujoco-mjx-lab_amd/csrc/model_host.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    // on the heap, exactly sized: the sanitizer sees any read or write past either struct
    std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
    std::unique_ptr<mjl::ModelF> f(new mjl::ModelF);
    FILE* fp = std::fopen(argv[a], "rb");
    const bool whole = fp && std::fread(d.get(), sizeof(mjlModelDesc), 1, fp) == 1 && std::fgetc(fp) == EOF;
    if (fp) std::fclose(fp);
    if (!whole) {
      std::fprintf(stderr, "%s: not a file of %zu bytes (one mjlModelDesc)\n", argv[a], sizeof(mjlModelDesc));
      return 2;
    }
    int nefc_max = 0, ncon_max = 0;
    std::string msg;
    const int rc = mjl::model_build(d.get(), *f, nefc_max, ncon_max, msg);
    std::printf("%s\trc=%d\tnefc_max=%d\tncon_max=%d\tsizeof_ModelF=%zu\tmsg=%s\n", argv[a], rc, nefc_max, ncon_max,
                sizeof(mjl::ModelF), msg.c_str());
  }
  return 0;
}
