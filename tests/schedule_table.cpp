// Stand-alone host program of tests/test_schedule_cpu.py: the schedule csrc/schedule.hpp chooses for every row of inputs
// on standard input, one name per line.  A row is
//   family wide pot64_tile N D logG mjhmc_mode L n_iter replay no_fuse no_compact fuse_below pot64_multipass
// with family one of dense / user / gaussian / rows / other and fuse_below a number or "-" (MJHMC_FUSE_BELOW not set).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../mjhmc_amd/csrc/schedule.hpp"

using namespace mjhmc;

static const char* schedule_name(Schedule s) {
  switch (s) {
    case Schedule::Multipass: return "Multipass";
    case Schedule::Fused: return "Fused";
    case Schedule::DenseParts: return "DenseParts";
    case Schedule::Compact: return "Compact";
    case Schedule::Plain: return "Plain";
  }
  return "?";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream row(line);
    std::string family, fuse_below;
    ScheduleInputs in;
    int wide, tile, mjhmc_mode, replay, no_fuse, no_compact, multipass;
    long long N;
    if (!(row >> family >> wide >> tile >> N >> in.D >> in.logG >> mjhmc_mode >> in.L >> in.n_iter >> replay >> no_fuse >>
          no_compact >> fuse_below >> multipass)) {
      std::fprintf(stderr, "bad row: %s\n", line.c_str());
      return 2;
    }
    if (family == "dense") in.family = EnergyFamily::Dense;
    else if (family == "user") in.family = EnergyFamily::User;
    else if (family == "gaussian") in.family = EnergyFamily::Gaussian;
    else if (family == "rows") in.family = EnergyFamily::Rows;
    else if (family == "other") in.family = EnergyFamily::Other;
    else return 2;
    in.wide = wide != 0;
    in.pot64_tile = tile != 0;
    in.N = N;
    in.mjhmc_mode = mjhmc_mode != 0;
    in.replay = replay != 0;
    in.no_fuse = no_fuse != 0;
    in.no_compact = no_compact != 0;
    if (fuse_below != "-") {
      in.fuse_below_set = true;
      in.fuse_below = std::stoll(fuse_below);
    }
    in.pot64_multipass = multipass != 0;
    std::puts(schedule_name(select_schedule(in)));
  }
  return 0;
}
