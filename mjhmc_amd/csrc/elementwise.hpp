// The elementwise energies' kernels, everything: the pieces by concern.
#pragma once
#include "sampler_args.hpp"
#include "lane_group.hpp"
#include "jump_math.hpp"
#include "energies.hpp"
#include "group_form.hpp"
#include "jump_process.hpp"
#include "jump_kernel.hpp"
#include "row_tile.hpp"
#include "row_form.hpp"
#include "step_kernel.hpp"
#include "launcher_decls.hpp"
#include "launchers.hpp"
