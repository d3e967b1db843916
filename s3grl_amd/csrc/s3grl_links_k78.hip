// Link kernels of sign_k = 7, 8 (s3grl_link_kernels.inl); s3grl_structure.hip's launch_links dispatches here.
#include "s3grl_link_kernels.inl"

namespace s3grl {
template s3grl_status launch_links_k<7>(s3grl_context*, const LinkArgs&, int64_t, const int32_t*);
template s3grl_status launch_links_k<8>(s3grl_context*, const LinkArgs&, int64_t, const int32_t*);
}  // namespace s3grl

S3GRL_DEFINE_TOUCH(links_k78)
