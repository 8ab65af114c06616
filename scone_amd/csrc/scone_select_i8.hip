// k_embed_select instantiations for table format SCONE_FMT_I8 (see scone_embed_select.h).
#include "scone_embed_select.h"

namespace scone_gather {
int launch_select_i8(scone_handle *h, const select_args &a, int out_dtype, hipStream_t s) {
  return launch_select_fmt<SCONE_FMT_I8>(h, a, out_dtype, s);
}
}  // namespace scone_gather
