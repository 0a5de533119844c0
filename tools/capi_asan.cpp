// Host-side argument checks of libmoe_hip.so under AddressSanitizer (SURVEY.md
// 5, "race detection / sanitizers"): every call below hands the C-ABI an
// invalid argument (NULL operand, bad shape, unknown option) and must come
// back with a non-zero code and a moe_last_error() message -- before any
// launch, so it needs no GPU.  Built and run by tests/test_capi_asan.py with
// the library and this driver compiled `-Xarch_host -fsanitize=address`
// (build_ext.py --asan); any out-of-bounds host access, use-after-free or leak
// in the checking / error paths fails the run.
#include <cstdio>
#include <cstring>

#include "../include/moe_hip.h"

static int g_fail = 0, g_n = 0;

static void expect_error(const char* what, int rc) {
  ++g_n;
  const char* msg = moe_last_error();
  if (rc == 0 || msg == nullptr || std::strlen(msg) == 0) {
    std::printf("FAIL %s: rc=%d msg=%s\n", what, rc, msg ? msg : "(null)");
    ++g_fail;
  } else {
    std::printf("ok   %-28s rc=%d  %s\n", what, rc, msg);
  }
}

int main() {
  // plausible-looking (never dereferenced) device pointers for the non-NULL arguments
  char buf[4096] __attribute__((aligned(256)));
  void* p = buf;
  auto* i32 = reinterpret_cast<int32_t*>(buf);
  auto* f32 = reinterpret_cast<float*>(buf);
  hipStream_t s = nullptr;
  expect_error("router_topk_fwd E=0", moe_router_topk_fwd(p, f32, nullptr, nullptr, 0, 16, 16, 256, 0, 1, 1, i32, f32,
                                                          f32, f32, i32, i32, f32, s));
  expect_error("router_topk_fwd d=100", moe_router_topk_fwd(p, f32, nullptr, nullptr, 0, 16, 16, 100, 8, 2, 1, i32,
                                                            f32, f32, f32, i32, i32, f32, s));
  expect_error("route_scan k=0", moe_route_scan(i32, 1, 0, 8, 0, i32, i32, i32, s));
  expect_error("permute_fwd d=7", moe_permute_fwd(p, i32, i32, i32, i32, 16, 7, 8, 2, 0, p, i32, s));
  expect_error("combine_fwd k=0", moe_combine_fwd(p, i32, f32, 16, 256, 0, p, s));
  expect_error("token_bwd d=100", moe_token_bwd(p, i32, f32, i32, f32, f32, f32, nullptr, nullptr, f32, 16, 100, 8,
                                                2, 1, p, f32, s));
  expect_error("token_bwd dw=NULL", moe_token_bwd(p, i32, f32, i32, f32, nullptr, f32, nullptr, nullptr, f32, 16, 256,
                                                  8, 2, 1, p, f32, s));
  expect_error("grouped_gemm N=100", moe_grouped_gemm(0, p, p, p, i32, 8, 64, 100, 256, 1, 0, nullptr, nullptr,
                                                      nullptr, s));
  expect_error("grouped_gemm bias epi, no bias", moe_grouped_gemm(0, p, p, p, i32, 8, 64, 1024, 256, 1, 1, nullptr,
                                                                  nullptr, nullptr, s));
  expect_error("grouped_gemm_gather G=0", moe_grouped_gemm_gather(0, p, i32, p, p, i32, 0, 64, 1024, 256, 1, 0,
                                                                  nullptr, nullptr, s));
  expect_error("wgrad_rows M=63", moe_grouped_gemm_wgrad_rows(0, p, p, p, nullptr, i32, 8, 63, 128, 0, 0, s));
  expect_error("bwd_pair epilogue=9", moe_grouped_gemm_bwd_pair(p, nullptr, nullptr, p, p, i32, 8, 64, 1024, 256, 9,
                                                                nullptr, p, nullptr, nullptr, p, nullptr, p, p,
                                                                1024, 256, 1, s));
  expect_error("expert_ffn_fwd d=128", moe_expert_ffn_fwd(0, p, nullptr, p, p, p, p, i32, 8, 64, 1024, 128, p, p,
                                                          nullptr, 0, s));
  expect_error("expert_ffn_fwd w1=NULL", moe_expert_ffn_fwd(0, p, nullptr, nullptr, p, p, p, i32, 8, 64, 1024, 256,
                                                            p, p, nullptr, 0, s));
  expect_error("expert_ffn_fwd fp8 dtype", moe_expert_ffn_fwd(1, p, nullptr, p, p, p, p, i32, 8, 64, 1024, 256, p,
                                                              p, nullptr, 0, s));
  expect_error("ep_compaction W=0", moe_ep_compaction(i32, i32, 0, 2, 16, 64, i32, i32, i32, s));
  expect_error("ep_compaction gather=NULL", moe_ep_compaction(i32, i32, 8, 2, 16, 64, nullptr, i32, i32, s));
  expect_error("quantize_mx K=31", moe_quantize_mx(p, 16, 31, p, p, s));
  expect_error("router_wgrad E=0", moe_router_wgrad(f32, p, nullptr, 1, 16, 0, 256, 0, f32, f32, nullptr, s));
  expect_error("aux_loss_fwd E=0", moe_aux_loss_fwd(f32, 1, 0, i32, 16, 2, 0.01f, 0.001f, f32, f32, s));
  expect_error("set_tuning unknown key", moe_set_tuning("no_such_knob", 1));
  expect_error("set_tuning bad value", moe_set_tuning("ksplit", 99));
  const float lr = 1e-4f;
  expect_error("adamw_step 0 groups", train_adamw_step(p, i32, 1, f32, f32, f32, f32, i32, &lr, 0, 0.f, 0.9f,
                                                       0.999f, 1e-8f, s));
  expect_error("adamw_ema_step ema=NULL", train_adamw_ema_step(p, i32, 1, f32, f32, f32, f32, i32, &lr, 1, 0.f, 0.9f,
                                                               0.999f, 1e-8f, nullptr, 0.5f, s));
  expect_error("adamw_ema_step decay=1", train_adamw_ema_step(p, i32, 1, f32, f32, f32, f32, i32, &lr, 1, 0.f, 0.9f,
                                                              0.999f, 1e-8f, f32, 1.0f, s));
  expect_error("ema_update misaligned ema", train_ema_update(p, i32, 1, f32 + 1, 0.5f, s));
  expect_error("ema_update decay<0", train_ema_update(p, i32, 1, f32, -0.1f, s));
  expect_error("grad_accum misaligned acc", train_grad_accum(p, i32, 1, f32 + 1, 1, s));
  expect_error("grad_accum acc=NULL", train_grad_accum(p, i32, 1, nullptr, 0, s));
  expect_error("grad_accum n_chunks<0", train_grad_accum(p, i32, -1, f32, 0, s));
  expect_error("augment_images Wp=62", train_augment_images(p, 0, 3 * 64 * 62, 64 * 62, 62, 1, p, 0, f32, 1, 64, 62, 40,
                                                            60, 0.447f, s));
  expect_error("augment_boxes M=2048", train_augment_boxes(f32, reinterpret_cast<int64_t*>(buf), i32, f32, 1, 2048,
                                                           64, 64, 40, 60, f32 + 64, reinterpret_cast<int64_t*>(buf) + 64,
                                                           i32 + 8, f32 + 8, s));
  const double* f64 = reinterpret_cast<const double*>(buf);
  uint8_t* u8 = reinterpret_cast<uint8_t*>(buf);
  expect_error("eval_match K=1025", rtdetr_eval_match(f32, f32, i32, f64, i32, i32, f64, 1, 1025, 4, 10, u8, s));
  expect_error("eval_match T=17", rtdetr_eval_match(f32, f32, i32, f64, i32, i32, f64, 1, 300, 4, 17, u8, s));
  expect_error("eval_match M=0", rtdetr_eval_match(f32, f32, i32, f64, i32, i32, f64, 1, 300, 0, 10, u8, s));
  expect_error("eval_match tp=NULL", rtdetr_eval_match(f32, f32, i32, f64, i32, i32, f64, 1, 300, 4, 10, nullptr, s));
  expect_error("eval_match_bands R=9",
               rtdetr_eval_match_bands(f32, f32, i32, f64, i32, i32, f64, f64, f64, 1, 300, 4, 10, 9, u8, s));
  expect_error("eval_match_bands R=0",
               rtdetr_eval_match_bands(f32, f32, i32, f64, i32, i32, f64, f64, f64, 1, 300, 4, 10, 0, u8, s));
  expect_error("eval_match_bands K=1025",
               rtdetr_eval_match_bands(f32, f32, i32, f64, i32, i32, f64, f64, f64, 1, 1025, 4, 10, 3, u8, s));
  expect_error("eval_match_bands bands=NULL",
               rtdetr_eval_match_bands(f32, f32, i32, f64, i32, i32, f64, f64, nullptr, 1, 300, 4, 10, 3, u8, s));
  expect_error("eval_match_bands code=NULL",
               rtdetr_eval_match_bands(f32, f32, i32, f64, i32, i32, f64, f64, f64, 1, 300, 4, 10, 3, nullptr, s));
  auto* i64 = reinterpret_cast<long long*>(buf);
  expect_error("route_stats T%tpi", moe_route_stats(i32, f32, i32, f32, i32, 6, 5, 12, 8, 2, i64, s));
  expect_error("route_stats E=65", moe_route_stats(i32, f32, i32, f32, i32, 6, 6, 12, 65, 2, i64, s));
  expect_error("route_stats k>E", moe_route_stats(i32, f32, i32, f32, i32, 6, 6, 12, 2, 3, i64, s));
  expect_error("route_stats k=9", moe_route_stats(i32, f32, i32, f32, i32, 6, 6, 12, 16, 9, i64, s));
  expect_error("route_stats n_ctx=0", moe_route_stats(i32, f32, i32, f32, i32, 0, 6, 12, 8, 2, i64, s));
  expect_error("route_stats ctx=NULL n_ctx=6", moe_route_stats(i32, f32, i32, f32, nullptr, 6, 6, 12, 8, 2, i64, s));
  expect_error("route_stats stats=NULL", moe_route_stats(i32, f32, i32, f32, i32, 6, 6, 12, 8, 2, nullptr, s));
  expect_error("router_topk_fwd_sel E=0", moe_router_topk_fwd_sel(p, f32, nullptr, nullptr, 0, 16, 16, 256, 0, 1, 1, f32,
                                                                  i32, f32, f32, f32, i32, i32, f32, s));
  expect_error("router_topk_fwd_sel d=100", moe_router_topk_fwd_sel(p, f32, nullptr, nullptr, 0, 16, 16, 100, 8, 2, 1,
                                                                    f32, i32, f32, f32, f32, i32, i32, f32, s));
  expect_error("router_topk_fwd_sel sel=NULL k>E", moe_router_topk_fwd_sel(p, f32, nullptr, nullptr, 0, 16, 16, 256, 2, 3,
                                                                           1, nullptr, i32, f32, f32, f32, i32, i32, f32,
                                                                           s));
  expect_error("balance_step E=0", moe_balance_step(buf, 2, 0, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step E=65", moe_balance_step(buf, 2, 65, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step L=-1", moe_balance_step(buf, -1, 8, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step table=NULL", moe_balance_step(nullptr, 2, 8, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step load=NULL", moe_balance_step(buf, 2, 8, nullptr, 1e-3f, 1, f32, s));
  expect_error("router_topk_fwd_selctx ctx=NULL", moe_router_topk_fwd_selctx(p, f32, nullptr, nullptr, 0, 16, 16, 256, 8, 2,
                                                                             1, f32, i32, f32, f32, f32, i32, i32, f32, s));
  expect_error("router_topk_fwd_selctx sel=NULL", moe_router_topk_fwd_selctx(p, f32, f32, i32, 6, 16, 16, 256, 8, 2, 1,
                                                                             nullptr, i32, f32, f32, f32, i32, i32, f32, s));
  expect_error("router_topk_fwd_selctx LDS", moe_router_topk_fwd_selctx(p, f32, f32, i32, 64, 16, 16, 256, 64, 2, 1, f32,
                                                                        i32, f32, f32, f32, i32, i32, f32, s));
  expect_error("balance_step_ctx E=65", moe_balance_step_ctx(buf, 2, 6, 65, 2, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step_ctx k>E", moe_balance_step_ctx(buf, 2, 6, 2, 3, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step_ctx C=0", moe_balance_step_ctx(buf, 2, 0, 8, 2, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step_ctx L=-1", moe_balance_step_ctx(buf, -1, 6, 8, 2, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step_ctx table=NULL", moe_balance_step_ctx(nullptr, 2, 6, 8, 2, i64, 1e-3f, 1, f32, s));
  expect_error("balance_step_ctx load=NULL", moe_balance_step_ctx(buf, 2, 6, 8, 2, nullptr, 1e-3f, 1, f32, s));
  expect_error("resize_pad src=NULL", rtdetr_resize_pad_u8(nullptr, i64, 1, 32, 32, 32, 32, f32, s));
  expect_error("resize_pad desc=NULL", rtdetr_resize_pad_u8(u8, nullptr, 1, 32, 32, 32, 32, f32, s));
  expect_error("resize_pad dst=NULL", rtdetr_resize_pad_u8(u8, i64, 1, 32, 32, 32, 32, nullptr, s));
  expect_error("resize_pad out_h=0", rtdetr_resize_pad_u8(u8, i64, 1, 0, 32, 32, 32, f32, s));
  expect_error("resize_pad out_w=-1", rtdetr_resize_pad_u8(u8, i64, 1, 32, -1, 32, 32, f32, s));
  expect_error("resize_pad pad_h<out_h", rtdetr_resize_pad_u8(u8, i64, 1, 33, 32, 32, 32, f32, s));
  expect_error("resize_pad pad_w<out_w", rtdetr_resize_pad_u8(u8, i64, 1, 32, 33, 32, 32, f32, s));
  expect_error("resize_pad B=-1", rtdetr_resize_pad_u8(u8, i64, -1, 32, 32, 32, 32, f32, s));
  ++g_n;
  if (rtdetr_resize_pad_u8(nullptr, nullptr, 0, 32, 32, 32, 32, nullptr, s) != 0) {  // B == 0: success, no launch
    std::printf("FAIL resize_pad B=0 must succeed\n");
    ++g_fail;
  }
  expect_error("nms_merge N=4097", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 4097, 0.25f, 0.5f, 1, 0, 300, f32, f32,
                                                    i32, i32, i32, s));
  expect_error("nms_merge max_det=0", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 0, f32, f32,
                                                       i32, i32, i32, s));
  expect_error("nms_merge max_det=1025", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 1025, f32,
                                                          f32, i32, i32, i32, s));
  expect_error("nms_merge B=1025", rtdetr_nms_merge(f32, f32, i32, nullptr, 1025, 64, 0.25f, 0.5f, 1, 0, 300, f32, f32,
                                                    i32, i32, i32, s));
  expect_error("nms_merge metric=2", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 2, 0, 300, f32, f32,
                                                      i32, i32, i32, s));
  expect_error("nms_merge thr=NaN", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 64, 0.25f, __builtin_nanf(""), 1, 0,
                                                     300, f32, f32, i32, i32, i32, s));
  expect_error("nms_merge boxes=NULL", rtdetr_nms_merge(nullptr, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, f32,
                                                        f32, i32, i32, i32, s));
  expect_error("nms_merge count=NULL", rtdetr_nms_merge(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, f32,
                                                        f32, i32, i32, nullptr, s));
  expect_error("nms_merge boxes misaligned", rtdetr_nms_merge(f32 + 1, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0,
                                                              300, f32, f32, i32, i32, i32, s));
  ++g_n;
  if (rtdetr_nms_merge(nullptr, nullptr, nullptr, nullptr, 0, 64, 0.25f, 0.5f, 1, 0, 300, nullptr, nullptr, nullptr,
                       nullptr, nullptr, s) != 0) {  // B == 0: success, no launch
    std::printf("FAIL nms_merge B=0 must succeed\n");
    ++g_fail;
  }
  const float nanf_ = __builtin_nanf("");
  expect_error("box_fuse N=4097", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 4097, 0.25f, 0.5f, 1, 0, 300, 0.55f,
                                                  nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse max_det=1025", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 1025, 0.55f,
                                                        nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse metric=2", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 2, 0, 300, 0.55f,
                                                    nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse thr=NaN", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, nanf_, 1, 0, 300, 0.55f,
                                                   nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse fuse_thr=NaN", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, nanf_,
                                                        nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse P=-1", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f, f32, -1,
                                                f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse P=65", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 65, 0.25f, 0.5f, 1, 0, 300, 0.55f, f32, 65,
                                                f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse N%P", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f, f32, 5,
                                               f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse windows=NULL P=4", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300,
                                                            0.55f, nullptr, 4, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse windows misaligned", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300,
                                                              0.55f, f32 + 1, 4, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse boxes=NULL", rtdetr_box_fuse(nullptr, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f,
                                                      nullptr, 0, f32, f32, i32, i32, i32, i32, s));
  expect_error("box_fuse members=NULL", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f,
                                                        nullptr, 0, f32, f32, i32, i32, i32, nullptr, s));
  expect_error("box_fuse count=NULL", rtdetr_box_fuse(f32, f32, i32, nullptr, 1, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f,
                                                      nullptr, 0, f32, f32, i32, i32, nullptr, i32, s));
  ++g_n;
  if (rtdetr_box_fuse(nullptr, nullptr, nullptr, nullptr, 0, 64, 0.25f, 0.5f, 1, 0, 300, 0.55f, nullptr, 0, nullptr,
                      nullptr, nullptr, nullptr, nullptr, nullptr, s) != 0) {  // B == 0: success, no launch
    std::printf("FAIL box_fuse B=0 must succeed\n");
    ++g_fail;
  }
  auto* c64 = reinterpret_cast<int64_t*>(buf);
  auto* d64 = reinterpret_cast<double*>(buf);
  // F, M, K, S, NG, NT, thr, then one operand replaced
  auto mot = [&](int F, int M, int K, int S, int NG, int NT, float thr, const float* gtb, int32_t* status) {
    return rtdetr_mot_eval(gtb, i32, i32, i32, f32, i32, i32, i32, i32, F, M, K, S, NG, NT, thr, i32, i32, i32, c64, d64,
                           i32, i32, i32, status, s);
  };
  expect_error("mot_eval K=1025", mot(1, 4, 1025, 1, 8, 8, 0.5f, f32, i32));
  expect_error("mot_eval M=257", mot(1, 257, 4, 1, 8, 8, 0.5f, f32, i32));
  expect_error("mot_eval M=0", mot(1, 0, 4, 1, 8, 8, 0.5f, f32, i32));
  expect_error("mot_eval NG=1025", mot(1, 4, 4, 1, 1025, 8, 0.5f, f32, i32));
  expect_error("mot_eval NT=4097", mot(1, 4, 4, 1, 8, 4097, 0.5f, f32, i32));
  expect_error("mot_eval F=1025", mot(1025, 4, 4, 1, 8, 8, 0.5f, f32, i32));
  expect_error("mot_eval S=0 with frames", mot(1, 4, 4, 0, 8, 8, 0.5f, f32, i32));
  expect_error("mot_eval thr=0", mot(1, 4, 4, 1, 8, 8, 0.f, f32, i32));
  expect_error("mot_eval thr=NaN", mot(1, 4, 4, 1, 8, 8, __builtin_nanf(""), f32, i32));
  expect_error("mot_eval gt_boxes=NULL", mot(1, 4, 4, 1, 8, 8, 0.5f, nullptr, i32));
  expect_error("mot_eval gt_boxes misaligned", mot(1, 4, 4, 1, 8, 8, 0.5f, f32 + 1, i32));
  expect_error("mot_eval status=NULL", mot(1, 4, 4, 1, 8, 8, 0.5f, f32, nullptr));
  ++g_n;
  if (mot(0, 4, 4, 0, 8, 8, 0.5f, nullptr, nullptr) != 0) {  // F == 0: success, no launch
    std::printf("FAIL mot_eval F=0 must succeed\n");
    ++g_fail;
  }
  // HOTA: F, M, K, S, NG, NT, thr, then one operand replaced
  auto hota_a = [&](int F, int M, int K, int S, int NG, int NT, float thr, const float* gtb, int32_t* status) {
    return rtdetr_hota_pass_a(gtb, i32, i32, i32, f32, i32, i32, i32, F, M, K, S, NG, NT, thr, c64, i32, i32, u8, status,
                              s);
  };
  auto hota_b = [&](int F, int M, int K, int S, int NG, int NT, const float* gtb, const double* alpha) {
    return rtdetr_hota_pass_b(gtb, i32, i32, i32, f32, i32, i32, i32, u8, F, M, K, S, NG, NT, f32, alpha, c64, i32, d64,
                              i32, s);
  };
  expect_error("hota_pass_a K=1025", hota_a(1, 4, 1025, 1, 8, 8, 0.5f, f32, i32));
  expect_error("hota_pass_a M=257", hota_a(1, 257, 4, 1, 8, 8, 0.5f, f32, i32));
  expect_error("hota_pass_a F=65537", hota_a(65537, 4, 4, 1, 8, 8, 0.5f, f32, i32));
  expect_error("hota_pass_a table over the budget", hota_a(1, 4, 4, 1, 1024, 2049, 0.5f, f32, i32));
  expect_error("hota_pass_a S * NG * NT over the budget", hota_a(1, 4, 4, 3, 1024, 1024, 0.5f, f32, i32));
  expect_error("hota_pass_a S=0 with frames", hota_a(1, 4, 4, 0, 8, 8, 0.5f, f32, i32));
  expect_error("hota_pass_a thr=NaN", hota_a(1, 4, 4, 1, 8, 8, __builtin_nanf(""), f32, i32));
  expect_error("hota_pass_a gt_boxes=NULL", hota_a(1, 4, 4, 1, 8, 8, 0.5f, nullptr, i32));
  expect_error("hota_pass_a gt_boxes misaligned", hota_a(1, 4, 4, 1, 8, 8, 0.5f, f32 + 1, i32));
  expect_error("hota_pass_a status=NULL", hota_a(1, 4, 4, 1, 8, 8, 0.5f, f32, nullptr));
  expect_error("hota_pass_b K=1025", hota_b(1, 4, 1025, 1, 8, 8, f32, d64));
  expect_error("hota_pass_b M=0", hota_b(1, 0, 4, 1, 8, 8, f32, d64));
  expect_error("hota_pass_b table over the budget", hota_b(1, 4, 4, 1, 1024, 2049, f32, d64));
  expect_error("hota_pass_b gt_boxes=NULL", hota_b(1, 4, 4, 1, 8, 8, nullptr, d64));
  expect_error("hota_pass_b alpha=NULL", hota_b(1, 4, 4, 1, 8, 8, f32, nullptr));
  expect_error("hota_pass_b alpha misaligned",
               hota_b(1, 4, 4, 1, 8, 8, f32, reinterpret_cast<const double*>(buf + 4)));
  expect_error("hota_gas table over the budget", rtdetr_hota_gas(c64, i32, i32, 1, 1024, 2049, f32, s));
  expect_error("hota_gas NG=0", rtdetr_hota_gas(c64, i32, i32, 1, 0, 8, f32, s));
  expect_error("hota_gas gas=NULL", rtdetr_hota_gas(c64, i32, i32, 1, 8, 8, nullptr, s));
  g_n += 3;
  if (hota_a(0, 4, 4, 0, 8, 8, 0.5f, nullptr, nullptr) != 0 || hota_b(0, 4, 4, 0, 8, 8, nullptr, nullptr) != 0 ||
      rtdetr_hota_gas(nullptr, nullptr, nullptr, 0, 8, 8, nullptr, s) != 0) {  // F == 0 / S == 0: success, no launch
    std::printf("FAIL hota F=0 / S=0 must succeed\n");
    ++g_fail;
  }
  // the tracker's parameter sweep: F, K, S, T, G, then one operand replaced
  auto sweep = [&](int F, int K, int S, int T, int G, const float* pf, const int32_t* pi, float* obox, float* tbox,
                   int32_t* orow) {
    return rtdetr_track_sweep(f32, f32, i32, nullptr, i32, i32, F, K, S, T, G, pf, pi, tbox, f32, i32, i32, i32, obox,
                              orow, i32, nullptr, s);
  };
  expect_error("track_sweep G=0", sweep(1, 8, 1, 4, 0, f32, i32, f32, f32, i32));
  expect_error("track_sweep G=1025", sweep(1, 8, 1, 4, 1025, f32, i32, f32, f32, i32));
  expect_error("track_sweep T=257", sweep(1, 8, 1, 257, 2, f32, i32, f32, f32, i32));
  expect_error("track_sweep T=0", sweep(1, 8, 1, 0, 2, f32, i32, f32, f32, i32));
  expect_error("track_sweep K=1025", sweep(1, 1025, 1, 4, 2, f32, i32, f32, f32, i32));
  expect_error("track_sweep F=1025", sweep(1025, 8, 1, 4, 2, f32, i32, f32, f32, i32));
  expect_error("track_sweep S=0 with frames", sweep(1, 8, 0, 4, 2, f32, i32, f32, f32, i32));
  expect_error("track_sweep params_f=NULL", sweep(1, 8, 1, 4, 2, nullptr, i32, f32, f32, i32));
  expect_error("track_sweep params_i=NULL", sweep(1, 8, 1, 4, 2, f32, nullptr, f32, f32, i32));
  expect_error("track_sweep out_row=NULL", sweep(1, 8, 1, 4, 2, f32, i32, f32, f32, nullptr));
  expect_error("track_sweep out_boxes misaligned", sweep(1, 8, 1, 4, 2, f32, i32, f32 + 1, f32, i32));
  expect_error("track_sweep trk_box misaligned", sweep(1, 8, 1, 4, 2, f32, i32, f32, f32 + 1, i32));
  ++g_n;
  if (sweep(0, 8, 0, 4, 2, f32, i32, nullptr, nullptr, nullptr) != 0) {  // F == 0: success, no launch
    std::printf("FAIL track_sweep F=0 must succeed\n");
    ++g_fail;
  }
  // the entries that take the association: assoc outside {0, 1}, the third table, the shared limits
  auto upd = [&](int K, int T, int assoc) {
    return rtdetr_track_update_assoc(f32, f32, i32, nullptr, i32, i32, 1, K, 1, T, 0.5f, 0.1f, 0.6f, 0.2f, 0.5f, 30, 2,
                                     0.5f, 0.25f, 0, f32, f32, i32, i32, i32, f32, i32, nullptr, assoc, s);
  };
  expect_error("track_update_assoc assoc=2", upd(8, 4, 2));
  expect_error("track_update_assoc assoc=-1", upd(8, 4, -1));
  expect_error("track_update_assoc K=1025", upd(1025, 4, 1));
  expect_error("track_update_assoc T=257", upd(8, 257, 1));
  auto sweep_a = [&](int K, int G, const int32_t* pa) {
    return rtdetr_track_sweep_assoc(f32, f32, i32, nullptr, i32, i32, 1, K, 1, 4, G, f32, i32, f32, f32, i32, i32, i32,
                                    f32, i32, i32, nullptr, pa, s);
  };
  expect_error("track_sweep_assoc params_assoc=NULL", sweep_a(8, 2, nullptr));
  expect_error("track_sweep_assoc G=0", sweep_a(8, 0, i32));
  expect_error("track_sweep_assoc K=1025", sweep_a(1025, 2, i32));
  std::printf("%d checks, %d failed\n", g_n, g_fail);
  return g_fail == 0 ? 0 : 1;
}
