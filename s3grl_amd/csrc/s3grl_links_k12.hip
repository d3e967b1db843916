// Link kernels of sign_k = 1, 2 (s3grl_link_kernels.inl); s3grl_structure.hip's launch_links dispatches here.
#include "s3grl_link_kernels.inl"

namespace s3grl {
template s3grl_status launch_links_k<1>(s3grl_context*, const LinkArgs&, int64_t, const int32_t*);
template s3grl_status launch_links_k<2>(s3grl_context*, const LinkArgs&, int64_t, const int32_t*);
}  // namespace s3grl

S3GRL_DEFINE_TOUCH(links_k12)
