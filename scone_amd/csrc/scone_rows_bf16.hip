// k_embed_rows instantiations for live rows of type SCONE_DT_BF16 (see scone_embed_rows.h).
#include "scone_embed_rows.h"

namespace scone_gather {
int launch_rows_bf16(scone_handle *h, const live_rows_view &live, const embed_args &a, int out_dtype, hipStream_t s) {
  return launch_rows_fmt<SCONE_FMT_BF16>(h, live, a, out_dtype, s);
}
}  // namespace scone_gather
