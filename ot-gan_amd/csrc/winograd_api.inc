// winograd_api.inc -- the functions of winograd.hip, declared inside namespace WINO_NS.  winograd.hip is compiled
// twice: wino_p2 = two scaled fp16 pieces per operand element, three MFMAs per product (default); wino_p3 = three
// bf16 pieces, 24 significand bits, six MFMAs (OTGAN_WINO_PIECES=3).  conv.hip includes this file once per namespace.
namespace WINO_NS {
bool winograd_enabled();
// accumulate: record = max(record, amax) (sub-slot 0) instead of overwriting all sub-slots
void wino_absmax(const float* x, long rows, int C, long ld, float* record, hipStream_t s, bool accumulate = false);
size_t wino_fwd_ws_floats(const WinoGeo& g);
size_t wino_dgrad_ws_floats(const WinoGeo& g);
size_t wino_wgrad_ws_floats(const WinoGeo& g);
size_t wino_x_operand_floats(const WinoGeo& g);      // 0: forward and weight gradient do not share the operand
size_t wino_s2_x_operand_floats(const WinoS2Geo& g);
size_t wino_filter_floats(const WinoGeo& g, int which);   // which: 0 forward (from weffT), 1 dgrad (from weff)
int wino_prepare_filters(const WinoGeo& g, int which, const float* w, long cls_stride, float* out, hipStream_t s);
int wino_fwd(const WinoGeo& g, const float* x, const float* weffT, long cls_stride, const float* bias, float* y,
             float* ws, hipStream_t s, const float* prep = nullptr);
int wino_dgrad(const WinoGeo& g, const float* dy, const float* weff, long cls_stride, float* dx, int lddx,
               int accumulate, float* ws, hipStream_t s, const float* prep = nullptr);
int wino_wgrad(const WinoGeo& g, const float* x, const float* dy, float* dweff, long cls_stride, float* ws,
               hipStream_t s, float* dw_unfolded5 = nullptr);
size_t wino_s2_fwd_ws_floats(const WinoS2Geo& g);
size_t wino_s2_dgrad_ws_floats(const WinoS2Geo& g);
size_t wino_s2_wgrad_ws_floats(const WinoS2Geo& g);
size_t wino_s2_filter_floats(const WinoS2Geo& g, int which);   // which: 0 forward (from wT), 1 dgrad (from w)
int wino_s2_prepare_filters(const WinoS2Geo& g, int which, const float* w, float* out, hipStream_t s);
int wino_s2_fwd(const WinoS2Geo& g, const float* x, const float* wT, const float* bias, float* y, float* ws,
                hipStream_t s, const float* prep = nullptr);
int wino_s2_dgrad(const WinoS2Geo& g, const float* dy, const float* w, const float* x, float* dx, int lddx,
                  int accumulate, float* ws, hipStream_t s, const float* prep = nullptr);
int wino_s2_wgrad(const WinoS2Geo& g, const float* x, const float* dy, float* dw, float* ws, hipStream_t s);
size_t wino_up3_fwd_ws_floats(const WinoUp3Geo& g);
size_t wino_up3_filter_floats(const WinoUp3Geo& g);
int wino_up3_prepare_filters(const WinoUp3Geo& g, const float* wT, float* out, hipStream_t s);
int wino_up3_fwd(const WinoUp3Geo& g, const float* x, const float* bias, float* y, float* ws, hipStream_t s,
                 const float* prep);
// the same operands from the raw weight-norm direction V (HWIO) and scale[Cout] = g * inv_norm, bit-identical to the ones made
// from the normalised copies (which is then never written); un-folded sources only (wino: which = 2 / 3), w_amax required
int wino_prepare_filters_raw(const WinoGeo& g, int which, const float* V, const float* scale, float* out, hipStream_t s);
int wino_s2_prepare_filters_raw(const WinoS2Geo& g, int which, const float* V, const float* scale, float* out, hipStream_t s);
int wino_up3_prepare_filters_raw(const WinoUp3Geo& g, const float* V, const float* scale, float* out, hipStream_t s);
}  // namespace WINO_NS
