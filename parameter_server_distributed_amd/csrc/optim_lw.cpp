// GPU dispatch of the layer-table apply: hands the gfx950 launchers of kernels/optim_lw.hip to the
// shared host code (optim_lw.h). Linked into the extension; left out of the host-only test programs.
#include "optim_lw.h"

namespace psd {

namespace {
const LwGpu kTable{&launch_lw_norms, &launch_lw_finalize, &launch_lw_apply};
const bool kRegistered = (lw_gpu() = &kTable, true);
}  // namespace

}  // namespace psd
