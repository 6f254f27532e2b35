// Restores from damaged copies of a small checkpoint; built with -fsanitize=address,undefined (Makefile).  Every
// artemis_sim_restore must either succeed or return NULL with a message -- a sanitizer report ends the program.
//   restart_reader <linear_wave.in> <work directory>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "artemis_driver.h"

static std::string slurp(const std::string &name) {
  std::ifstream in(name, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}
static void spit(const std::string &name, const std::string &bytes) {
  std::ofstream out(name, std::ios::binary | std::ios::trunc);
  out.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string deck = slurp(argv[1]), work = argv[2];
  if (deck.empty()) return 2;
  const char *over[] = {"parthenon/mesh/nx1=16", "parthenon/mesh/nx2=1", "parthenon/mesh/nx3=1", "parthenon/meshblock/nx1=16",
                        "parthenon/meshblock/nx2=1", "parthenon/meshblock/nx3=1", "problem/along_x1=true", "problem/amp=1.0e-6",
                        "problem/wave_flag=0", "problem/vflow=0.0", "parthenon/time/nlim=100"};
  artemis_sim_t *s = artemis_sim_create(deck.c_str(), sizeof over / sizeof *over, over, nullptr);
  if (!s || artemis_sim_evolve(s, 3) != 3) return std::printf("create: %s\n", artemis_sim_last_error()), 1;
  const std::string good = work + "/good", bad = work + "/bad";
  if (artemis_sim_save(s, good.c_str())) return std::printf("save: %s\n", artemis_sim_last_error()), 1;
  artemis_sim_destroy(s);
  const std::string raw = slurp(good + "/part-00000.bin");
  const size_t payload = 6 * (16 + 4) * sizeof(double); // one block of one gas species
  if (raw.size() <= payload) return std::printf("part too small\n"), 1;
  mkdir(bad.c_str(), 0777);
  long ok = 0, refused = 0;
  auto attempt = [&](const std::string &bytes) {
    spit(bad + "/part-00000.bin", bytes);
    artemis_sim_t *r = artemis_sim_restore(bad.c_str(), 0, nullptr, nullptr);
    if (!r) {
      if (!artemis_sim_last_error()[0]) std::printf("refused without a message\n"), std::exit(1);
      ++refused;
      return;
    }
    if (artemis_sim_evolve(r, 1) != 1) std::printf("restored but cannot step: %s\n", artemis_sim_last_error()), std::exit(1);
    artemis_sim_destroy(r);
    ++ok;
  };
  attempt(raw);
  if (ok != 1) return std::printf("the intact copy was refused: %s\n", artemis_sim_last_error()), 1;
  for (size_t cut = 0; cut < raw.size(); cut += 97) attempt(raw.substr(0, cut));
  const size_t head = raw.size() - payload; // header, global header, directory, checksum
  for (int q = 0; q < 500; ++q) {
    std::string b = raw;
    const size_t at = head * static_cast<size_t>(q) / 500;
    b[at] = static_cast<char>(b[at] ^ (1 << (q % 8)));
    attempt(b);
  }
  if (ok != 1) return std::printf("%ld damaged copies were accepted\n", ok - 1), 1;
  std::printf("restart_reader: ok (%ld refused cleanly)\n", refused);
  return 0;
}
