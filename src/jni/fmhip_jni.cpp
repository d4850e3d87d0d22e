// fmhip_jni.cpp — the JNI layer of net.finmath.hip.Native: ONE function per C-ABI function of include/fmhip.h, no logic
// beyond argument marshalling ("JNI layer = one Java_net_finmath_hip_Native_* function per C-ABI function").
//
// UNCOMPILED against a real JDK / UNTESTED in a JVM in this repository: the build image has no JDK (no jni.h).  CMakeLists.txt at
// the repository root builds it only when find_package(JNI) succeeds.  What IS done on every run of the CPU test suite
// (tests/test_jni_binding_cpu.py): this file is compiled against a hand-written declaration stub of <jni.h> (tests/jni_stub: the
// types and the JNIEnv members used here) and linked against libfmhip.so — every C++ error and every mismatch with
// include/fmhip.h shows — and the set of functions here, the native methods of java/net/finmath/hip/Native.java and the exports
// of the header are checked to be the same set.
//
// Marshalling rules: every array is accessed with Get/Release<Type>ArrayElements (may copy; other JNI calls stay legal) — no
// critical region is held around an engine call (an upload or a read-back synchronises with the device and may compile a
// kernel: a pinned array would stall the collector for that long); EVERY array length is checked against what the C function
// will read or write before it is called (FMHIP_ERR_INVALID_ARGUMENT otherwise: a short array from Java must never become a
// native overrun); out-parameters are 1-element (or documented-length) arrays; a null array where the C function accepts NULL
// is passed as NULL.
#include <jni.h>
#include <cstdint>
#include <string>
#include <vector>
#include "fmhip.h"

namespace {

// RAII access to the elements of a primitive Java array (may be null).  Pin<T> = Get/Release<Type>ArrayElements: may copy, and
// other JNI calls (further arrays, GetArrayLength) stay legal while it is held — used wherever several arrays travel together.
template <typename T> struct ArrayOps;
template <> struct ArrayOps<jint>    { static jint*    get(JNIEnv* e, jarray a) { return e->GetIntArrayElements((jintArray)a, nullptr); }       static void put(JNIEnv* e, jarray a, jint* p, jint m)    { e->ReleaseIntArrayElements((jintArray)a, p, m); } };
template <> struct ArrayOps<jlong>   { static jlong*   get(JNIEnv* e, jarray a) { return e->GetLongArrayElements((jlongArray)a, nullptr); }     static void put(JNIEnv* e, jarray a, jlong* p, jint m)   { e->ReleaseLongArrayElements((jlongArray)a, p, m); } };
template <> struct ArrayOps<jdouble> { static jdouble* get(JNIEnv* e, jarray a) { return e->GetDoubleArrayElements((jdoubleArray)a, nullptr); } static void put(JNIEnv* e, jarray a, jdouble* p, jint m) { e->ReleaseDoubleArrayElements((jdoubleArray)a, p, m); } };
template <> struct ArrayOps<jfloat>  { static jfloat*  get(JNIEnv* e, jarray a) { return e->GetFloatArrayElements((jfloatArray)a, nullptr); }   static void put(JNIEnv* e, jarray a, jfloat* p, jint m)  { e->ReleaseFloatArrayElements((jfloatArray)a, p, m); } };
template <typename T>
struct Pin {
    JNIEnv* env; jarray arr; T* p; jint mode; jsize len;
    Pin(JNIEnv* e, jarray a, jint release_mode = 0) : env(e), arr(a), p(nullptr), mode(release_mode), len(a ? e->GetArrayLength(a) : 0) { if (a) p = ArrayOps<T>::get(e, a); }
    ~Pin() { if (arr && p) ArrayOps<T>::put(env, arr, p, mode); }
    jsize length() const { return len; }
};
// fmhip_prog_op[] from the parallel arrays of Native.programCreate / programSource
// (false: an operand array is missing or shorter than the opcode array)
bool program_ops(JNIEnv* env, jintArray opcode, jintArray a, jintArray b, jintArray c, jdoubleArray scalar, std::vector<fmhip_prog_op>& ops) {
    const jsize n = opcode ? env->GetArrayLength(opcode) : 0;
    ops.assign((size_t)n, fmhip_prog_op{});
    if (n == 0) return true;
    Pin<jint> po(env, opcode, JNI_ABORT), pa(env, a, JNI_ABORT), pb(env, b, JNI_ABORT), pc(env, c, JNI_ABORT);
    Pin<jdouble> ps(env, scalar, JNI_ABORT);
    if (!po.p || !pa.p || !pb.p || !pc.p || pa.length() < n || pb.length() < n || pc.length() < n || (ps.p && ps.length() < n)) return false;
    for (jsize i = 0; i < n; ++i) ops[(size_t)i] = { po.p[i], pa.p[i], pb.p[i], pc.p[i], ps.p ? ps.p[i] : 0.0 };
    return true;
}

inline void set1(JNIEnv* env, jintArray arr, jint v) { if (arr && env->GetArrayLength(arr) > 0) env->SetIntArrayRegion(arr, 0, 1, &v); }
inline void set1(JNIEnv* env, jlongArray arr, jlong v) { if (arr && env->GetArrayLength(arr) > 0) env->SetLongArrayRegion(arr, 0, 1, &v); }

} // namespace

#define FMJ(ret, name) extern "C" JNIEXPORT ret JNICALL Java_net_finmath_hip_Native_##name

// ---------------------------------------------------------------- lifecycle
FMJ(jint, init)(JNIEnv*, jclass, jint deviceIndex) { return fmhip_init(deviceIndex); }
FMJ(jint, initDevices)(JNIEnv* env, jclass, jintArray devices) {
    Pin<jint> pd(env, devices, JNI_ABORT);
    if (!pd.p) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_init_devices((const int*)pd.p, pd.length());
}
FMJ(jint, deviceCount)(JNIEnv* env, jclass, jintArray count) {
    if (!count || env->GetArrayLength(count) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    int c = 0;
    const int st = fmhip_device_count(&c);
    if (st == FMHIP_OK) { const jint v = c; env->SetIntArrayRegion(count, 0, 1, &v); }
    return st;
}
FMJ(jint, setThreadEngines)(JNIEnv* env, jclass, jint enabled, jintArray previous) {
    int prev = 0;
    const int st = fmhip_set_thread_engines(enabled, &prev);
    if (st == FMHIP_OK && previous && env->GetArrayLength(previous) >= 1) { const jint v = prev; env->SetIntArrayRegion(previous, 0, 1, &v); }
    return st;
}
FMJ(jint, shutdown)(JNIEnv*, jclass) { return fmhip_shutdown(); }
FMJ(jint, isInitialized)(JNIEnv*, jclass) { return fmhip_is_initialized(); }
FMJ(jint, abiVersion)(JNIEnv*, jclass) { return fmhip_abi_version(); }
FMJ(jstring, lastError)(JNIEnv* env, jclass) { return env->NewStringUTF(fmhip_last_error()); }
FMJ(jint, deviceInfo)(JNIEnv* env, jclass, jobjectArray name, jintArray computeUnits, jlongArray hbmBytes) {
    char buf[256] = { 0 }; int cus = 0; int64_t hbm = 0;
    const int st = fmhip_device_info(buf, (int)sizeof buf, &cus, &hbm);
    if (st == FMHIP_OK) {
        if (name && env->GetArrayLength(name) > 0) env->SetObjectArrayElement(name, 0, env->NewStringUTF(buf));
        set1(env, computeUnits, (jint)cus); set1(env, hbmBytes, (jlong)hbm);
    }
    return st;
}
FMJ(jint, synchronize)(JNIEnv*, jclass) { return fmhip_synchronize(); }
FMJ(jint, getStream)(JNIEnv* env, jclass, jlongArray stream) {
    void* s = nullptr;
    const int st = fmhip_get_stream(&s);
    if (st == FMHIP_OK) set1(env, stream, (jlong)(intptr_t)s);
    return st;
}

// ---------------------------------------------------------------- vectors
FMJ(jlong, vecCreateFromDouble)(JNIEnv* env, jclass, jdoubleArray values) {
    Pin<jdouble> p(env, values, JNI_ABORT);
    fmhip_vec out = 0;
    return fmhip_vec_create_from_double(p.p, p.length(), &out) == FMHIP_OK ? (jlong)out : 0;
}
FMJ(jlong, vecCreateFromFloat)(JNIEnv* env, jclass, jfloatArray values) {
    Pin<jfloat> p(env, values, JNI_ABORT);
    fmhip_vec out = 0;
    return fmhip_vec_create_from_float(p.p, p.length(), &out) == FMHIP_OK ? (jlong)out : 0;
}
FMJ(jlong, vecCreateFilled)(JNIEnv*, jclass, jlong n, jdouble value) { fmhip_vec out = 0; return fmhip_vec_create_filled(n, value, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jlong, vecCreateUninitialized)(JNIEnv*, jclass, jlong n) { fmhip_vec out = 0; return fmhip_vec_create_uninitialized(n, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jint, vecRetain)(JNIEnv*, jclass, jlong v) { return fmhip_vec_retain(v); }
FMJ(jint, vecRelease)(JNIEnv*, jclass, jlong v) { return fmhip_vec_release(v); }
FMJ(jint, vecSize)(JNIEnv* env, jclass, jlong v, jlongArray size) {
    int64_t n = 0;
    const int st = fmhip_vec_size(v, &n);
    if (st == FMHIP_OK) set1(env, size, (jlong)n);
    return st;
}
FMJ(jint, vecReadDouble)(JNIEnv* env, jclass, jlong v, jdoubleArray out) { Pin<jdouble> p(env, out); return fmhip_vec_read_double(v, p.p, p.length()); }     // (the engine checks the length against the vector's)
FMJ(jint, vecReadFloat)(JNIEnv* env, jclass, jlong v, jfloatArray out) { Pin<jfloat> p(env, out); return fmhip_vec_read_float(v, p.p, p.length()); }
FMJ(jint, vecDevicePtr)(JNIEnv* env, jclass, jlong v, jlongArray devicePointer) {
    void* ptr = nullptr;
    const int st = fmhip_vec_device_ptr(v, &ptr);
    if (st == FMHIP_OK) set1(env, devicePointer, (jlong)(intptr_t)ptr);
    return st;
}

// ---------------------------------------------------------------- element-wise operations (the hot path: no allocation, no array)
FMJ(jlong, callV1s0)(JNIEnv*, jclass, jint opcode, jlong a) { fmhip_vec out = 0; return fmhip_call_v1s0(opcode, a, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jlong, callV1s1)(JNIEnv*, jclass, jint opcode, jlong a, jdouble s) { fmhip_vec out = 0; return fmhip_call_v1s1(opcode, a, s, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jlong, callV2s0)(JNIEnv*, jclass, jint opcode, jlong a, jlong b) { fmhip_vec out = 0; return fmhip_call_v2s0(opcode, a, b, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jlong, callV2s1)(JNIEnv*, jclass, jint opcode, jlong a, jlong b, jdouble s) { fmhip_vec out = 0; return fmhip_call_v2s1(opcode, a, b, s, &out) == FMHIP_OK ? (jlong)out : 0; }
FMJ(jlong, callV3s0)(JNIEnv*, jclass, jint opcode, jlong a, jlong b, jlong c) { fmhip_vec out = 0; return fmhip_call_v3s0(opcode, a, b, c, &out) == FMHIP_OK ? (jlong)out : 0; }

// ---------------------------------------------------------------- lazy fusion front-end
FMJ(jint, setFusion)(JNIEnv* env, jclass, jint enabled, jintArray previous) { int prev = 0; const int st = fmhip_set_fusion(enabled, &prev); if (st == FMHIP_OK) set1(env, previous, prev); return st; }
FMJ(jint, flush)(JNIEnv*, jclass) { return fmhip_flush(); }
FMJ(jint, setStepGrouping)(JNIEnv* env, jclass, jint steps, jintArray previous) { int prev = 0; const int st = fmhip_set_step_grouping(steps, &prev); if (st == FMHIP_OK) set1(env, previous, prev); return st; }
FMJ(jint, fusionHold)(JNIEnv* env, jclass, jint hold, jintArray previous) { int prev = 0; const int st = fmhip_fusion_hold(hold, &prev); if (st == FMHIP_OK) set1(env, previous, prev); return st; }
FMJ(jint, graphClone)(JNIEnv* env, jclass, jlongArray roots, jint nCopies, jlongArray leafFrom, jlongArray leafTo, jdoubleArray scalars, jint nScalars, jlongArray out) {
    Pin<jlong> pr(env, roots, JNI_ABORT), pf(env, leafFrom, JNI_ABORT), pt(env, leafTo, JNI_ABORT), po(env, out); Pin<jdouble> ps(env, scalars, JNI_ABORT);
    if (nCopies < 0 || nScalars < 0 || !pr.p || !po.p || (int64_t)pt.length() < (int64_t)pf.length() * nCopies || (int64_t)po.length() < (int64_t)pr.length() * nCopies ||
        (ps.p && (int64_t)ps.length() < (int64_t)nScalars * nCopies)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_graph_clone((const fmhip_vec*)pr.p, pr.length(), nCopies, (const fmhip_vec*)pf.p, (const fmhip_vec*)pt.p, pf.length(), ps.p, nScalars, (fmhip_vec*)po.p);
}
FMJ(jint, graphScalars)(JNIEnv* env, jclass, jlongArray roots, jdoubleArray scalarsOut, jintArray count) {
    int n = 0, st;
    { Pin<jlong> pr(env, roots, JNI_ABORT); Pin<jdouble> ps(env, scalarsOut); st = fmhip_graph_scalars((const fmhip_vec*)pr.p, pr.length(), ps.p, ps.length(), &n); }     // capacity = the array's own length
    if (st == FMHIP_OK) set1(env, count, n);
    return st;
}
FMJ(jint, setMathMode)(JNIEnv* env, jclass, jint mode, jintArray previous) { int prev = 0; const int st = fmhip_set_math_mode(mode, &prev); if (st == FMHIP_OK) set1(env, previous, prev); return st; }

// ---------------------------------------------------------------- reductions
FMJ(jint, reduceMoments)(JNIEnv* env, jclass, jlong v, jdouble shift, jdoubleArray moments4) {
    fmhip_moments m;
    const int st = fmhip_reduce_moments(v, shift, &m);
    if (st == FMHIP_OK && moments4 && env->GetArrayLength(moments4) >= 4) { const jdouble d[4] = { m.sum, m.sumsq, m.min, m.max }; env->SetDoubleArrayRegion(moments4, 0, 4, d); }
    return st;
}
FMJ(jint, reduceMomentsDevice)(JNIEnv*, jclass, jlong v, jdouble shift, jlong deviceOut) { return fmhip_reduce_moments_device(v, shift, (void*)(intptr_t)deviceOut); }
FMJ(jint, reduceMomentsBatch)(JNIEnv* env, jclass, jlongArray vectors, jdoubleArray shifts, jdoubleArray moments4PerVector) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jdouble> ps(env, shifts, JNI_ABORT); Pin<jdouble> pm(env, moments4PerVector);
    static_assert(sizeof(fmhip_moments) == 4 * sizeof(double), "moments travel as 4 doubles");
    if (!pv.p || !pm.p || (int64_t)pm.length() < 4 * (int64_t)pv.length() || (ps.p && ps.length() < pv.length())) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_reduce_moments_batch((const fmhip_vec*)pv.p, pv.length(), ps.p, (fmhip_moments*)pm.p);
}
// ---------------------------------------------------------------- order statistics
FMJ(jint, selectRanksBatch)(JNIEnv* env, jclass, jlongArray vectors, jlongArray ranks, jdoubleArray valuesOut) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jlong> pr(env, ranks, JNI_ABORT); Pin<jdouble> po(env, valuesOut);
    static_assert(sizeof(jlong) == sizeof(int64_t), "ranks travel as 64-bit integers");
    if (!pv.p || !pr.p || !po.p || (int64_t)po.length() < (int64_t)pv.length() * (int64_t)pr.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_select_ranks_batch((const fmhip_vec*)pv.p, pv.length(), (const int64_t*)pr.p, pr.length(), po.p);
}
FMJ(jint, rankSumsBatch)(JNIEnv* env, jclass, jlongArray vectors, jlong rankFrom, jlong rankTo, jdoubleArray sumsOut) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!pv.p || !po.p || po.length() < pv.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_rank_sums_batch((const fmhip_vec*)pv.p, pv.length(), rankFrom, rankTo, po.p);
}
FMJ(jint, countNotAbove)(JNIEnv* env, jclass, jlong v, jdoubleArray bounds, jlongArray countsOut) {
    Pin<jdouble> pb(env, bounds, JNI_ABORT); Pin<jlong> po(env, countsOut);
    if (!pb.p || !po.p || po.length() < pb.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_count_not_above(v, pb.p, pb.length(), (int64_t*)po.p);
}
// ---------------------------------------------------------------- cross moments
FMJ(jint, crossMoments)(JNIEnv* env, jclass, jlongArray x, jlongArray y, jdoubleArray sumsOut) {
    Pin<jlong> px(env, x, JNI_ABORT); Pin<jlong> py(env, y, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!px.p || !po.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nx = px.length(), ny = py.p ? py.length() : 0;
    if ((int64_t)po.length() < nx * (nx + 1) / 2 + nx * ny) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_cross_moments((const fmhip_vec*)px.p, (int)nx, ny ? (const fmhip_vec*)py.p : nullptr, (int)ny, po.p);
}
FMJ(jint, crossMomentsWide)(JNIEnv* env, jclass, jlongArray x, jlongArray y, jdoubleArray sumsOut) {
    Pin<jlong> px(env, x, JNI_ABORT); Pin<jlong> py(env, y, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!px.p || !po.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nx = px.length(), ny = py.p ? py.length() : 0;
    if ((int64_t)po.length() < nx * (nx + 1) / 2 + nx * ny) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_cross_moments_wide((const fmhip_vec*)px.p, (int)nx, ny ? (const fmhip_vec*)py.p : nullptr, (int)ny, po.p);
}
// ---------------------------------------------------------------- localized regression: cross moments per bin of a key, the piecewise estimate
FMJ(jint, binnedCrossMoments)(JNIEnv* env, jclass, jlong key, jdoubleArray bounds, jlongArray x, jlongArray y, jlongArray countsOut, jdoubleArray sumsOut) {
    Pin<jdouble> pb(env, bounds, JNI_ABORT); Pin<jlong> px(env, x, JNI_ABORT); Pin<jlong> py(env, y, JNI_ABORT); Pin<jlong> pc(env, countsOut); Pin<jdouble> po(env, sumsOut);
    if (!px.p || !pc.p || !po.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nb = (pb.p ? pb.length() : 0) + 1, nx = px.length(), ny = py.p ? py.length() : 0;
    if ((int64_t)pc.length() < nb || (int64_t)po.length() < nb * (nx * (nx + 1) / 2 + nx * ny)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_binned_cross_moments(key, pb.p, (int)nb, (const fmhip_vec*)px.p, (int)nx, ny ? (const fmhip_vec*)py.p : nullptr, (int)ny, (int64_t*)pc.p, po.p);
}
// columns: nX (nY) columns of key.length floats each, one after the other; bit i of onesMask: x_i is the constant 1 and its column is not read
static bool binned_columns(const jfloat* flat, int64_t flatLength, int64_t n, int count, int onesMask, std::vector<const float*>& out) {
    if (count < 0 || count > 8) return false;
    for (int i = 0; i < count; ++i) {
        if ((onesMask >> i) & 1) { out.push_back(nullptr); continue; }
        if (!flat || flatLength < (int64_t)(i + 1) * n) return false;
        out.push_back(flat + (int64_t)i * n);
    }
    return true;
}
FMJ(jint, binnedCrossMomentsHost)(JNIEnv* env, jclass, jfloatArray key, jdoubleArray bounds, jfloatArray xColumns, jint nX, jint onesMask, jfloatArray yColumns, jint nY, jlongArray countsOut, jdoubleArray sumsOut) {
    Pin<jfloat> pk(env, key, JNI_ABORT); Pin<jdouble> pb(env, bounds, JNI_ABORT); Pin<jfloat> px(env, xColumns, JNI_ABORT); Pin<jfloat> py(env, yColumns, JNI_ABORT); Pin<jlong> pc(env, countsOut); Pin<jdouble> po(env, sumsOut);
    if (!pk.p || !pc.p || !po.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pk.length(), nb = (pb.p ? pb.length() : 0) + 1;
    std::vector<const float*> xs, ys;
    if (!binned_columns(px.p, px.p ? px.length() : 0, n, nX, onesMask, xs) || !binned_columns(py.p, py.p ? py.length() : 0, n, nY, 0, ys)) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)pc.length() < nb || (int64_t)po.length() < nb * ((int64_t)nX * (nX + 1) / 2 + (int64_t)nX * nY)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_binned_cross_moments_host(pk.p, n, pb.p, (int)nb, xs.data(), nX, nY ? ys.data() : nullptr, nY, (int64_t*)pc.p, po.p);
}
FMJ(jint, binnedEvaluate)(JNIEnv* env, jclass, jlong key, jdoubleArray bounds, jlongArray x, jdoubleArray coefficients, jlongArray out) {
    Pin<jdouble> pb(env, bounds, JNI_ABORT); Pin<jlong> px(env, x, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT);
    if (!px.p || !pc.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nb = (pb.p ? pb.length() : 0) + 1, nx = px.length();
    if ((int64_t)pc.length() < nb * nx) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0;
    const int st = fmhip_binned_evaluate(key, pb.p, (int)nb, (const fmhip_vec*)px.p, (int)nx, pc.p, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
FMJ(jint, binnedEvaluateHost)(JNIEnv* env, jclass, jfloatArray key, jdoubleArray bounds, jfloatArray xColumns, jint nX, jint onesMask, jdoubleArray coefficients, jfloatArray out) {
    Pin<jfloat> pk(env, key, JNI_ABORT); Pin<jdouble> pb(env, bounds, JNI_ABORT); Pin<jfloat> px(env, xColumns, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT); Pin<jfloat> po(env, out);
    if (!pk.p || !pc.p || !po.p) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pk.length(), nb = (pb.p ? pb.length() : 0) + 1;
    std::vector<const float*> xs;
    if (!binned_columns(px.p, px.p ? px.length() : 0, n, nX, onesMask, xs)) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)pc.length() < nb * nX || (int64_t)po.length() < n) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_binned_evaluate_host(pk.p, n, pb.p, (int)nb, xs.data(), nX, pc.p, po.p);
}
// ---------------------------------------------------------------- sort on the device
FMJ(jint, sortByKey)(JNIEnv* env, jclass, jlong key, jlongArray values, jlongArray sortedKeyOut, jlongArray sortedValuesOut) {
    Pin<jlong> pv(env, values, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv > 8 || (nv > 0 && (!sortedValuesOut || env->GetArrayLength(sortedValuesOut) < nv)) || (sortedKeyOut && env->GetArrayLength(sortedKeyOut) < 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec k = 0, out[8] = { 0 };
    const int st = fmhip_sort_by_key(key, (const fmhip_vec*)pv.p, (int)nv, sortedKeyOut ? &k : nullptr, out);
    if (st == FMHIP_OK) {
        set1(env, sortedKeyOut, (jlong)k);
        if (nv > 0) { jlong o[8]; for (int i = 0; i < nv; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(sortedValuesOut, 0, (jsize)nv, o); }
    }
    return st;
}
FMJ(jint, argsort)(JNIEnv* env, jclass, jlong key, jlongArray permutationOut) {
    int64_t n = 0;
    const int sz = fmhip_vec_size(key, &n);
    if (sz != FMHIP_OK) return sz;
    Pin<jlong> po(env, permutationOut);
    if (!po.p || (int64_t)po.length() < n) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_argsort(key, (int64_t*)po.p);
}
FMJ(jint, argsortHost)(JNIEnv* env, jclass, jfloatArray key, jlongArray permutationOut) {
    Pin<jfloat> pk(env, key, JNI_ABORT); Pin<jlong> po(env, permutationOut);
    if (!pk.p || !po.p || po.length() < pk.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_argsort_host(pk.p, pk.length(), (int64_t*)po.p);
}
FMJ(jint, rankScores)(JNIEnv* env, jclass, jlong key, jlongArray out) {
    fmhip_vec h = 0;
    const int st = fmhip_rank_scores(key, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
FMJ(jint, vecReadElements)(JNIEnv* env, jclass, jlong v, jlongArray positions, jdoubleArray out) {
    Pin<jlong> pp(env, positions, JNI_ABORT); Pin<jdouble> po(env, out);
    if (!pp.p || !po.p || po.length() < pp.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_vec_read_elements(v, (const int64_t*)pp.p, (int)pp.length(), po.p);
}
// ---------------------------------------------------------------- prefix sums on the device
FMJ(jint, prefixSums)(JNIEnv* env, jclass, jlong v, jint mode, jlongArray out, jdoubleArray totalOutOrNull) {
    if (!out || env->GetArrayLength(out) < 1 || (totalOutOrNull && env->GetArrayLength(totalOutOrNull) < 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0; double total = 0.0;
    const int st = fmhip_prefix_sums(v, (int)mode, &h, &total);
    if (st == FMHIP_OK) { set1(env, out, (jlong)h); if (totalOutOrNull) env->SetDoubleArrayRegion(totalOutOrNull, 0, 1, &total); }
    return st;
}
FMJ(jint, prefixSumsAt)(JNIEnv* env, jclass, jlong v, jlongArray positions, jdoubleArray sumsOut) {
    Pin<jlong> pp(env, positions, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!pp.p || !po.p || po.length() < pp.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_prefix_sums_at(v, (const int64_t*)pp.p, (int)pp.length(), po.p);
}
FMJ(jint, prefixSearch)(JNIEnv* env, jclass, jlong v, jdoubleArray thresholds, jboolean relative, jlongArray positionsOut, jdoubleArray sumsOut, jdoubleArray totalOutOrNull) {
    if (totalOutOrNull && env->GetArrayLength(totalOutOrNull) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    double total = 0.0;
    int st;
    {
        Pin<jdouble> pt(env, thresholds, JNI_ABORT); Pin<jlong> pp(env, positionsOut); Pin<jdouble> ps(env, sumsOut);
        if (!pt.p || !pp.p || !ps.p || pp.length() < pt.length() || ps.length() < pt.length()) return FMHIP_ERR_INVALID_ARGUMENT;
        st = fmhip_prefix_search(v, pt.p, (int)pt.length(), relative ? 1 : 0, (int64_t*)pp.p, ps.p, &total);
    }
    if (st == FMHIP_OK && totalOutOrNull) env->SetDoubleArrayRegion(totalOutOrNull, 0, 1, &total);
    return st;
}
FMJ(jint, prefixSumsHost)(JNIEnv* env, jclass, jfloatArray v, jdoubleArray prefixOut) {
    Pin<jfloat> pv(env, v, JNI_ABORT); Pin<jdouble> po(env, prefixOut);
    if (!pv.p || !po.p || po.length() < pv.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_prefix_sums_host(pv.p, pv.length(), po.p);
}
// ---------------------------------------------------------------- resampling on the device
FMJ(jint, resample)(JNIEnv* env, jclass, jlong weights, jint scheme, jlong m, jdouble offset, jlong uniforms, jlongArray values, jlongArray valuesOut, jlongArray ancestorsOutOrNull,
                    jdoubleArray totalOutOrNull) {
    Pin<jlong> pv(env, values, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv > 8 || (nv > 0 && (!valuesOut || env->GetArrayLength(valuesOut) < nv)) || (ancestorsOutOrNull && env->GetArrayLength(ancestorsOutOrNull) < 1)
        || (totalOutOrNull && env->GetArrayLength(totalOutOrNull) < 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec a = 0, out[8] = { 0 };
    double total = 0.0;
    const int st = fmhip_resample((fmhip_vec)weights, (int)scheme, (int64_t)m, (double)offset, (fmhip_vec)uniforms, (const fmhip_vec*)pv.p, (int)nv, out, ancestorsOutOrNull ? &a : nullptr, &total);
    if (st == FMHIP_OK) {
        if (nv > 0) { jlong o[8]; for (int i = 0; i < nv; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(valuesOut, 0, (jsize)nv, o); }
        set1(env, ancestorsOutOrNull, (jlong)a);
        if (totalOutOrNull) env->SetDoubleArrayRegion(totalOutOrNull, 0, 1, &total);
    }
    return st;
}
FMJ(jint, resampleHost)(JNIEnv* env, jclass, jfloatArray weightsOrNull, jlong n, jint scheme, jlong m, jdouble offset, jfloatArray uniformsOrNull, jfloatArray valueColumns, jint nValues,
                        jfloatArray outColumns, jlongArray ancestorsOutOrNull, jdoubleArray totalOutOrNull) {
    if (totalOutOrNull && env->GetArrayLength(totalOutOrNull) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    double total = 0.0;
    int st;
    {
        Pin<jfloat> pw(env, weightsOrNull, JNI_ABORT); Pin<jfloat> pu(env, uniformsOrNull, JNI_ABORT); Pin<jfloat> pv(env, valueColumns, JNI_ABORT); Pin<jfloat> po(env, outColumns);
        Pin<jlong> pa(env, ancestorsOutOrNull);
        if (n < 1 || m < 1 || nValues < 0 || nValues > 8 || (pw.p && (int64_t)pw.length() < (int64_t)n) || (pu.p && (int64_t)pu.length() < (int64_t)m)
            || (pa.p && (int64_t)pa.length() < (int64_t)m)) return FMHIP_ERR_INVALID_ARGUMENT;
        if (nValues > 0 && (!pv.p || !po.p || (int64_t)pv.length() < (int64_t)nValues * n || (int64_t)po.length() < (int64_t)nValues * m)) return FMHIP_ERR_INVALID_ARGUMENT;
        const float* in[8] = { nullptr }; float* columns[8] = { nullptr };
        for (int i = 0; i < nValues; ++i) { in[i] = pv.p + (int64_t)i * n; columns[i] = po.p + (int64_t)i * m; }
        st = fmhip_resample_host(pw.p, (int64_t)n, (int)scheme, (int64_t)m, (double)offset, pu.p, in, (int)nValues, columns, (int64_t*)pa.p, &total);
    }
    if (st == FMHIP_OK && totalOutOrNull) env->SetDoubleArrayRegion(totalOutOrNull, 0, 1, &total);
    return st;
}
// ---------------------------------------------------------------- selection on the device
FMJ(jint, compress)(JNIEnv* env, jclass, jlong mask, jlongArray valuesOrNull, jlongArray valuesOutOrNull, jlongArray positionsOutOrNull, jlongArray countOutOrNull) {
    Pin<jlong> pv(env, valuesOrNull, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv > 8 || (nv > 0 && (!valuesOutOrNull || env->GetArrayLength(valuesOutOrNull) < nv)) || (positionsOutOrNull && env->GetArrayLength(positionsOutOrNull) < 1)
        || (countOutOrNull && env->GetArrayLength(countOutOrNull) < 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec positions = 0, out[8] = { 0 };
    int64_t count = 0;
    const int st = fmhip_compress((fmhip_vec)mask, (const fmhip_vec*)pv.p, (int)nv, out, positionsOutOrNull ? &positions : nullptr, &count);
    if (st == FMHIP_OK) {
        if (nv > 0) { jlong o[8]; for (int i = 0; i < nv; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(valuesOutOrNull, 0, (jsize)nv, o); }
        set1(env, positionsOutOrNull, (jlong)positions);
        set1(env, countOutOrNull, (jlong)count);
    }
    return st;
}
FMJ(jint, expand)(JNIEnv* env, jclass, jlong mask, jlongArray values, jdouble fill, jlongArray valuesOut) {
    Pin<jlong> pv(env, values, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv < 1 || nv > 8 || !valuesOut || env->GetArrayLength(valuesOut) < nv) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec out[8] = { 0 };
    const int st = fmhip_expand((fmhip_vec)mask, (const fmhip_vec*)pv.p, (int)nv, (double)fill, out);
    if (st == FMHIP_OK) { jlong o[8]; for (int i = 0; i < nv; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(valuesOut, 0, (jsize)nv, o); }
    return st;
}
FMJ(jint, gather)(JNIEnv* env, jclass, jlong index, jlongArray values, jlongArray valuesOut) {
    Pin<jlong> pv(env, values, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv < 1 || nv > 8 || !valuesOut || env->GetArrayLength(valuesOut) < nv) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec out[8] = { 0 };
    const int st = fmhip_gather((fmhip_vec)index, (const fmhip_vec*)pv.p, (int)nv, out);
    if (st == FMHIP_OK) { jlong o[8]; for (int i = 0; i < nv; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(valuesOut, 0, (jsize)nv, o); }
    return st;
}
FMJ(jint, compressHost)(JNIEnv* env, jclass, jfloatArray mask, jfloatArray valueColumns, jint nValues, jfloatArray outColumns, jlongArray positionsOutOrNull, jlongArray countOutOrNull) {
    if (countOutOrNull && env->GetArrayLength(countOutOrNull) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    int64_t count = 0;
    int st;
    {
        Pin<jfloat> pm(env, mask, JNI_ABORT); Pin<jfloat> pv(env, valueColumns, JNI_ABORT); Pin<jfloat> po(env, outColumns); Pin<jlong> pp(env, positionsOutOrNull);
        const int64_t n = pm.p ? (int64_t)pm.length() : 0;
        if (n < 1 || nValues < 0 || nValues > 8 || (pp.p && (int64_t)pp.length() < n)) return FMHIP_ERR_INVALID_ARGUMENT;
        if (nValues > 0 && (!pv.p || !po.p || (int64_t)pv.length() < (int64_t)nValues * n || (int64_t)po.length() < (int64_t)nValues * n)) return FMHIP_ERR_INVALID_ARGUMENT;
        const float* in[8] = { nullptr }; float* columns[8] = { nullptr };
        for (int i = 0; i < nValues; ++i) { in[i] = pv.p + (int64_t)i * n; columns[i] = po.p + (int64_t)i * n; }
        st = fmhip_compress_host(pm.p, n, in, (int)nValues, columns, (int64_t*)pp.p, &count);
    }
    if (st == FMHIP_OK) set1(env, countOutOrNull, (jlong)count);
    return st;
}
FMJ(jint, expandHost)(JNIEnv* env, jclass, jfloatArray mask, jfloatArray valueColumns, jint nValues, jlong nValueElements, jdouble fill, jfloatArray outColumns) {
    Pin<jfloat> pm(env, mask, JNI_ABORT); Pin<jfloat> pv(env, valueColumns, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    const int64_t n = pm.p ? (int64_t)pm.length() : 0, c = (int64_t)nValueElements;
    if (n < 1 || c < 0 || nValues < 1 || nValues > 8 || !pv.p || !po.p || (int64_t)pv.length() < (int64_t)nValues * c || (int64_t)po.length() < (int64_t)nValues * n) return FMHIP_ERR_INVALID_ARGUMENT;
    const float* in[8] = { nullptr }; float* columns[8] = { nullptr };
    for (int i = 0; i < nValues; ++i) { in[i] = pv.p + (int64_t)i * c; columns[i] = po.p + (int64_t)i * n; }
    return fmhip_expand_host(pm.p, n, in, (int)nValues, c, (double)fill, columns);
}
FMJ(jint, gatherHost)(JNIEnv* env, jclass, jfloatArray index, jfloatArray valueColumns, jint nValues, jlong n, jfloatArray outColumns) {
    Pin<jfloat> pi(env, index, JNI_ABORT); Pin<jfloat> pv(env, valueColumns, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    const int64_t m = pi.p ? (int64_t)pi.length() : 0;
    if (m < 1 || n < 1 || nValues < 1 || nValues > 8 || !pv.p || !po.p || (int64_t)pv.length() < (int64_t)nValues * (int64_t)n || (int64_t)po.length() < (int64_t)nValues * m) return FMHIP_ERR_INVALID_ARGUMENT;
    const float* in[8] = { nullptr }; float* columns[8] = { nullptr };
    for (int i = 0; i < nValues; ++i) { in[i] = pv.p + (int64_t)i * (int64_t)n; columns[i] = po.p + (int64_t)i * m; }
    return fmhip_gather_host(pi.p, m, in, (int)nValues, (int64_t)n, columns);
}
// ---------------------------------------------------------------- reduce by key on the device
static int groupOutputs(jint mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }
FMJ(jint, groupSums)(JNIEnv* env, jclass, jlong index, jlong m, jlongArray valuesOrNull, jint mask, jlongArray countsOutOrNull, jlongArray outsOrNull, jlongArray ungroupedOutOrNull) {
    Pin<jlong> pv(env, valuesOrNull, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (mask < 0 || mask > 7 || nv > 4) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n_out = nv * groupOutputs(mask);
    if ((n_out > 0 && (!outsOrNull || env->GetArrayLength(outsOrNull) < n_out)) || (countsOutOrNull && env->GetArrayLength(countsOutOrNull) < 1)
        || (ungroupedOutOrNull && env->GetArrayLength(ungroupedOutOrNull) < 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec counts = 0, out[12] = { 0 };
    int64_t ungrouped = 0;
    const int st = fmhip_group_sums((fmhip_vec)index, (int64_t)m, (const fmhip_vec*)pv.p, (int)nv, (uint32_t)mask, countsOutOrNull ? &counts : nullptr, out, ungroupedOutOrNull ? &ungrouped : nullptr);
    if (st == FMHIP_OK) {
        if (n_out > 0) { jlong o[12]; for (int i = 0; i < n_out; ++i) o[i] = (jlong)out[i]; env->SetLongArrayRegion(outsOrNull, 0, (jsize)n_out, o); }
        set1(env, countsOutOrNull, (jlong)counts);
        set1(env, ungroupedOutOrNull, (jlong)ungrouped);
    }
    return st;
}
FMJ(jint, groupSumsHost)(JNIEnv* env, jclass, jfloatArray index, jlong m, jfloatArray valueColumns, jint nValues, jint mask, jfloatArray countsOutOrNull, jfloatArray outColumns, jlongArray ungroupedOutOrNull) {
    if (ungroupedOutOrNull && env->GetArrayLength(ungroupedOutOrNull) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    int64_t ungrouped = 0;
    int st;
    {
        Pin<jfloat> pi(env, index, JNI_ABORT); Pin<jfloat> pv(env, valueColumns, JNI_ABORT); Pin<jfloat> pc(env, countsOutOrNull); Pin<jfloat> po(env, outColumns);
        const int64_t n = pi.p ? (int64_t)pi.length() : 0;
        if (n < 1 || m < 1 || m > (int64_t(1) << 24) || nValues < 0 || nValues > 4 || mask < 0 || mask > 7 || (pc.p && (int64_t)pc.length() < (int64_t)m)) return FMHIP_ERR_INVALID_ARGUMENT;
        const int per = groupOutputs(mask);
        if (nValues > 0 && (!pv.p || !po.p || (int64_t)pv.length() < (int64_t)nValues * n || (int64_t)po.length() < (int64_t)nValues * per * (int64_t)m)) return FMHIP_ERR_INVALID_ARGUMENT;
        const float* in[4] = { nullptr }; float* columns[12] = { nullptr };
        for (int i = 0; i < nValues; ++i) in[i] = pv.p + (int64_t)i * n;
        for (int i = 0; i < nValues * per; ++i) columns[i] = po.p + (int64_t)i * (int64_t)m;
        st = fmhip_group_sums_host(pi.p, n, (int64_t)m, in, (int)nValues, (uint32_t)mask, pc.p, columns, ungroupedOutOrNull ? &ungrouped : nullptr);
    }
    if (st == FMHIP_OK) set1(env, ungroupedOutOrNull, (jlong)ungrouped);
    return st;
}
// ---------------------------------------------------------------- tabulated functions on the device
FMJ(jint, tableBuild)(JNIEnv* env, jclass, jdoubleArray knots, jdoubleArray values, jint interpolation, jint extrapolation, jint derivative, jdoubleArray coefficientsOut) {
    Pin<jdouble> pk(env, knots, JNI_ABORT); Pin<jdouble> pv(env, values, JNI_ABORT); Pin<jdouble> po(env, coefficientsOut);
    if (!pk.p || !pv.p || !po.p || pv.length() < pk.length() || (int64_t)po.length() < ((int64_t)pk.length() + 1) * 4) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_table_build(pk.p, pv.p, (int)pk.length(), (int)interpolation, (int)extrapolation, (int)derivative, po.p);
}
FMJ(jint, tableApply)(JNIEnv* env, jclass, jlong x, jdoubleArray knots, jdoubleArray coefficients, jint nTables, jlongArray out) {
    Pin<jdouble> pk(env, knots, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT);
    if (!pk.p || !pc.p || !out || nTables < 1 || nTables > 4 || env->GetArrayLength(out) < nTables) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)pc.length() < (int64_t)nTables * ((int64_t)pk.length() + 1) * 4) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h[4] = { 0, 0, 0, 0 };
    const int st = fmhip_table_apply(x, pk.p, (int)pk.length(), pc.p, (int)nTables, h);
    if (st == FMHIP_OK) { jlong o[4]; for (int f = 0; f < nTables; ++f) o[f] = (jlong)h[f]; env->SetLongArrayRegion(out, 0, (jsize)nTables, o); }
    return st;
}
FMJ(jint, tableApplyHost)(JNIEnv* env, jclass, jfloatArray x, jdoubleArray knots, jdoubleArray coefficients, jint nTables, jfloatArray outColumns) {
    Pin<jfloat> px(env, x, JNI_ABORT); Pin<jdouble> pk(env, knots, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    if (!px.p || !pk.p || !pc.p || !po.p || nTables < 1 || nTables > 4) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = px.length();
    if ((int64_t)pc.length() < (int64_t)nTables * ((int64_t)pk.length() + 1) * 4 || (int64_t)po.length() < (int64_t)nTables * n) return FMHIP_ERR_INVALID_ARGUMENT;
    float* columns[4] = { nullptr, nullptr, nullptr, nullptr };
    for (int f = 0; f < nTables; ++f) columns[f] = po.p + (int64_t)f * n;
    return fmhip_table_apply_host(px.p, n, pk.p, (int)pk.length(), pc.p, (int)nTables, columns);
}
// ---------------------------------------------------------------- kernel regression: kernel-weighted local moments at a grid of points of a key
static int64_t kernel_entries(int order, int64_t ny) { return order == 0 ? 1 + ny : 3 + 2 * ny; }
FMJ(jint, kernelMoments)(JNIEnv* env, jclass, jlong key, jdoubleArray points, jdoubleArray bandwidths, jint kernel, jint order, jlongArray y, jdoubleArray sumsOut) {
    Pin<jdouble> pp(env, points, JNI_ABORT); Pin<jdouble> pb(env, bandwidths, JNI_ABORT); Pin<jlong> py(env, y, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!pp.p || !pb.p || !po.p || pb.length() < pp.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t q = pp.length(), ny = py.p ? py.length() : 0;
    if (ny > 4 || (order != 0 && order != 1) || (int64_t)po.length() < q * kernel_entries(order, ny)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_kernel_moments(key, pp.p, pb.p, (int)q, (int)kernel, (int)order, ny ? (const fmhip_vec*)py.p : nullptr, (int)ny, po.p);
}
FMJ(jint, kernelMomentsHost)(JNIEnv* env, jclass, jfloatArray key, jdoubleArray points, jdoubleArray bandwidths, jint kernel, jint order, jfloatArray yColumns, jint nY, jdoubleArray sumsOut) {
    Pin<jfloat> pk(env, key, JNI_ABORT); Pin<jdouble> pp(env, points, JNI_ABORT); Pin<jdouble> pb(env, bandwidths, JNI_ABORT); Pin<jfloat> py(env, yColumns, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!pk.p || !pp.p || !pb.p || !po.p || pb.length() < pp.length() || nY < 0 || nY > 4 || (order != 0 && order != 1)) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pk.length(), q = pp.length();
    std::vector<const float*> ys;
    if (!binned_columns(py.p, py.p ? py.length() : 0, n, nY, 0, ys)) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)po.length() < q * kernel_entries(order, nY)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_kernel_moments_host(pk.p, n, pp.p, pb.p, (int)q, (int)kernel, (int)order, nY ? ys.data() : nullptr, nY, po.p);
}
// ---------------------------------------------------------------- nested simulation: block moments and the repeat
FMJ(jint, blockMoments)(JNIEnv* env, jclass, jlongArray vs, jlong block, jint mask, jlongArray outs) {
    Pin<jlong> pv(env, vs, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv < 1 || nv > 4 || mask < 1 || mask > 7 || !outs) return FMHIP_ERR_INVALID_ARGUMENT;
    const int total = (int)nv * ((mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1));
    if (env->GetArrayLength(outs) < total) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h[12] = { 0 };
    const int st = fmhip_block_moments((const fmhip_vec*)pv.p, (int)nv, (int64_t)block, (uint32_t)mask, h);
    if (st == FMHIP_OK) { jlong o[12]; for (int k = 0; k < total; ++k) o[k] = (jlong)h[k]; env->SetLongArrayRegion(outs, 0, (jsize)total, o); }
    return st;
}
FMJ(jint, blockMomentsHost)(JNIEnv* env, jclass, jfloatArray v, jlong block, jint mask, jfloatArray outColumns) {
    Pin<jfloat> pv(env, v, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    if (!pv.p || !po.p || block < 1 || mask < 1 || mask > 7) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pv.length(), columns = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1);
    if ((int64_t)po.length() < columns * (n / (int64_t)block)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_block_moments_host(pv.p, n, (int64_t)block, (uint32_t)mask, po.p);
}
FMJ(jint, vecRepeat)(JNIEnv* env, jclass, jlong v, jlong each, jlong times, jlongArray out) {
    if (!out || env->GetArrayLength(out) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0;
    const int st = fmhip_vec_repeat(v, (int64_t)each, (int64_t)times, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
// ---------------------------------------------------------------- block order statistics and the block sort
FMJ(jint, blockOrderStatistics)(JNIEnv* env, jclass, jlongArray vs, jlong block, jlongArray ranks, jlongArray rangeFrom, jlongArray rangeTo, jlongArray outs) {
    Pin<jlong> pv(env, vs, JNI_ABORT); Pin<jlong> pr(env, ranks, JNI_ABORT); Pin<jlong> pf(env, rangeFrom, JNI_ABORT); Pin<jlong> pt(env, rangeTo, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0, nr = pr.p ? pr.length() : 0, ng = pf.p ? pf.length() : 0;
    if (nv < 1 || nv > 4 || nr > 8 || ng > 4 || nr + ng < 1 || (int64_t)(pt.p ? pt.length() : 0) != ng || !outs) return FMHIP_ERR_INVALID_ARGUMENT;
    const int total = (int)(nv * (nr + ng));
    if (env->GetArrayLength(outs) < total) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h[48] = { 0 };
    const int st = fmhip_block_order_statistics((const fmhip_vec*)pv.p, (int)nv, (int64_t)block, (const int64_t*)pr.p, (int)nr, (const int64_t*)pf.p, (const int64_t*)pt.p, (int)ng, h);
    if (st == FMHIP_OK) { jlong o[48]; for (int k = 0; k < total; ++k) o[k] = (jlong)h[k]; env->SetLongArrayRegion(outs, 0, (jsize)total, o); }
    return st;
}
FMJ(jint, blockOrderStatisticsHost)(JNIEnv* env, jclass, jfloatArray v, jlong block, jlongArray ranks, jlongArray rangeFrom, jlongArray rangeTo, jfloatArray outColumns) {
    Pin<jfloat> pv(env, v, JNI_ABORT); Pin<jlong> pr(env, ranks, JNI_ABORT); Pin<jlong> pf(env, rangeFrom, JNI_ABORT); Pin<jlong> pt(env, rangeTo, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    const int64_t nr = pr.p ? pr.length() : 0, ng = pf.p ? pf.length() : 0;
    if (!pv.p || !po.p || block < 1 || nr > 8 || ng > 4 || nr + ng < 1 || (int64_t)(pt.p ? pt.length() : 0) != ng) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pv.length();
    if ((int64_t)po.length() < (nr + ng) * (n / (int64_t)block)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_block_order_statistics_host(pv.p, n, (int64_t)block, (const int64_t*)pr.p, (int)nr, (const int64_t*)pf.p, (const int64_t*)pt.p, (int)ng, po.p);
}
FMJ(jint, blockSort)(JNIEnv* env, jclass, jlong v, jlong block, jlongArray out) {
    if (!out || env->GetArrayLength(out) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0;
    const int st = fmhip_block_sort(v, (int64_t)block, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
FMJ(jint, blockSortHost)(JNIEnv* env, jclass, jfloatArray v, jlong block, jfloatArray out) {
    Pin<jfloat> pv(env, v, JNI_ABORT); Pin<jfloat> po(env, out);
    if (!pv.p || !po.p || po.length() < pv.length()) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_block_sort_host(pv.p, pv.length(), (int64_t)block, po.p);
}
// ---------------------------------------------------------------- order statistics across vectors and the selection behind their index
FMJ(jint, crossOrderStatistics)(JNIEnv* env, jclass, jlongArray vs, jintArray ranks, jint outputs, jlongArray outs) {
    Pin<jlong> pv(env, vs, JNI_ABORT); Pin<jint> pr(env, ranks, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0, nr = pr.p ? pr.length() : 0;
    if (nv < 1 || nv > 32 || nr < 1 || nr > 32 || outputs < 1 || outputs > 3 || !outs) return FMHIP_ERR_INVALID_ARGUMENT;
    const int total = (int)(nr * ((outputs & 1) + ((outputs >> 1) & 1)));
    if (env->GetArrayLength(outs) < total) return FMHIP_ERR_INVALID_ARGUMENT;
    int r[32];
    for (int64_t j = 0; j < nr; ++j) r[j] = (int)pr.p[j];
    fmhip_vec h[64] = { 0 };
    const int st = fmhip_cross_order_statistics((const fmhip_vec*)pv.p, (int)nv, r, (int)nr, (int)outputs, h);
    if (st == FMHIP_OK) { jlong o[64]; for (int k = 0; k < total; ++k) o[k] = (jlong)h[k]; env->SetLongArrayRegion(outs, 0, (jsize)total, o); }
    return st;
}
FMJ(jint, crossOrderStatisticsHost)(JNIEnv* env, jclass, jfloatArray vsColumns, jint nVs, jintArray ranks, jint outputs, jfloatArray outColumns) {
    Pin<jfloat> pv(env, vsColumns, JNI_ABORT); Pin<jint> pr(env, ranks, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    const int64_t nr = pr.p ? pr.length() : 0;
    if (!pv.p || !po.p || nVs < 1 || nVs > 32 || nr < 1 || nr > 32 || outputs < 1 || outputs > 3 || pv.length() % nVs != 0) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pv.length() / nVs;
    const int total = (int)(nr * ((outputs & 1) + ((outputs >> 1) & 1)));
    if ((int64_t)po.length() < (int64_t)total * n) return FMHIP_ERR_INVALID_ARGUMENT;
    int r[32];
    for (int64_t j = 0; j < nr; ++j) r[j] = (int)pr.p[j];
    const float* in[32]; float* columns[64];
    for (int i = 0; i < nVs; ++i) in[i] = pv.p + (int64_t)i * n;
    for (int k = 0; k < total; ++k) columns[k] = po.p + (int64_t)k * n;
    return fmhip_cross_order_statistics_host(in, (int)nVs, n, r, (int)nr, (int)outputs, columns);
}
FMJ(jint, crossSelect)(JNIEnv* env, jclass, jlong index, jlongArray vs, jlongArray out) {
    Pin<jlong> pv(env, vs, JNI_ABORT);
    const int64_t nv = pv.p ? pv.length() : 0;
    if (nv < 1 || nv > 32 || !out || env->GetArrayLength(out) < 1) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0;
    const int st = fmhip_cross_select(index, (const fmhip_vec*)pv.p, (int)nv, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
FMJ(jint, crossSelectHost)(JNIEnv* env, jclass, jfloatArray index, jfloatArray vsColumns, jint nVs, jfloatArray out) {
    Pin<jfloat> pi(env, index, JNI_ABORT); Pin<jfloat> pv(env, vsColumns, JNI_ABORT); Pin<jfloat> po(env, out);
    if (!pi.p || !pv.p || !po.p || nVs < 1 || nVs > 32) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = pi.length();
    if ((int64_t)pv.length() != n * nVs || (int64_t)po.length() < n) return FMHIP_ERR_INVALID_ARGUMENT;
    const float* in[32];
    for (int i = 0; i < nVs; ++i) in[i] = pv.p + (int64_t)i * n;
    return fmhip_cross_select_host(pi.p, in, (int)nVs, n, po.p);
}
// ---------------------------------------------------------------- named functions and option formulas per path
FMJ(jint, functionApply)(JNIEnv* env, jclass, jlong x, jintArray kinds, jlongArray out) {
    Pin<jint> pk(env, kinds, JNI_ABORT);
    const jsize count = pk.length();
    if (!pk.p || !out || count < 1 || count > 4 || env->GetArrayLength(out) < count) return FMHIP_ERR_INVALID_ARGUMENT;
    int k[4] = { 0, 0, 0, 0 };
    for (jsize f = 0; f < count; ++f) k[f] = (int)pk.p[f];
    fmhip_vec h[4] = { 0, 0, 0, 0 };
    const int st = fmhip_function_apply(x, k, (int)count, h);
    if (st == FMHIP_OK) { jlong o[4]; for (jsize f = 0; f < count; ++f) o[f] = (jlong)h[f]; env->SetLongArrayRegion(out, 0, count, o); }
    return st;
}
FMJ(jint, functionApplyHost)(JNIEnv* env, jclass, jfloatArray x, jintArray kinds, jfloatArray outColumns) {
    Pin<jfloat> px(env, x, JNI_ABORT); Pin<jint> pk(env, kinds, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    const jsize count = pk.length();
    if (!px.p || !pk.p || !po.p || count < 1 || count > 4) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = px.length();
    if ((int64_t)po.length() < (int64_t)count * n) return FMHIP_ERR_INVALID_ARGUMENT;
    int k[4] = { 0, 0, 0, 0 };
    float* columns[4] = { nullptr, nullptr, nullptr, nullptr };
    for (jsize f = 0; f < count; ++f) { k[f] = (int)pk.p[f]; columns[f] = po.p + (int64_t)f * n; }
    return fmhip_function_apply_host(px.p, n, k, (int)count, columns);
}
FMJ(jint, optionFormula)(JNIEnv* env, jclass, jint model, jlong forward, jdouble forwardScalar, jlong volatility, jdouble volatilityScalar, jlong payoffUnit, jdouble payoffUnitScalar,
                         jdouble maturity, jdouble strike, jint outputs, jlongArray out) {
    if (!out || outputs < 1 || outputs > 7) return FMHIP_ERR_INVALID_ARGUMENT;
    const jsize count = (jsize)((outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1));
    if (env->GetArrayLength(out) < count) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h[3] = { 0, 0, 0 };
    const int st = fmhip_option_formula((int)model, forward, forwardScalar, volatility, volatilityScalar, payoffUnit, payoffUnitScalar, maturity, strike, (int)outputs, h);
    if (st == FMHIP_OK) { jlong o[3]; for (jsize f = 0; f < count; ++f) o[f] = (jlong)h[f]; env->SetLongArrayRegion(out, 0, count, o); }
    return st;
}
FMJ(jint, optionFormulaHost)(JNIEnv* env, jclass, jint model, jfloatArray forwardOrNull, jdouble forwardScalar, jfloatArray volatilityOrNull, jdouble volatilityScalar,
                             jfloatArray payoffUnitOrNull, jdouble payoffUnitScalar, jint n, jdouble maturity, jdouble strike, jint outputs, jfloatArray outColumns) {
    Pin<jfloat> pf(env, forwardOrNull, JNI_ABORT); Pin<jfloat> pv(env, volatilityOrNull, JNI_ABORT); Pin<jfloat> pn(env, payoffUnitOrNull, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    if (!po.p || n < 1 || outputs < 1 || outputs > 7) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((forwardOrNull && (!pf.p || pf.length() < n)) || (volatilityOrNull && (!pv.p || pv.length() < n)) || (payoffUnitOrNull && (!pn.p || pn.length() < n))) return FMHIP_ERR_INVALID_ARGUMENT;
    const int count = (outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1);
    if ((int64_t)po.length() < (int64_t)count * n) return FMHIP_ERR_INVALID_ARGUMENT;
    float* columns[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < count; ++f) columns[f] = po.p + (int64_t)f * n;
    return fmhip_option_formula_host((int)model, pf.p, forwardScalar, pv.p, volatilityScalar, pn.p, payoffUnitScalar, (int64_t)n, maturity, strike, (int)outputs, columns);
}
// ---------------------------------------------------------------- implied volatility per path: the inverse of optionFormula's value in the volatility
FMJ(jint, impliedVolatility)(JNIEnv* env, jclass, jint model, jlong price, jdouble priceScalar, jlong forward, jdouble forwardScalar, jlong payoffUnit, jdouble payoffUnitScalar,
                             jdouble maturity, jdouble strike, jint outputs, jlongArray out) {
    if (!out || outputs < 1 || outputs > 7) return FMHIP_ERR_INVALID_ARGUMENT;
    const jsize count = (jsize)((outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1));
    if (env->GetArrayLength(out) < count) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h[3] = { 0, 0, 0 };
    const int st = fmhip_implied_volatility((int)model, price, priceScalar, forward, forwardScalar, payoffUnit, payoffUnitScalar, maturity, strike, (int)outputs, h);
    if (st == FMHIP_OK) { jlong o[3]; for (jsize f = 0; f < count; ++f) o[f] = (jlong)h[f]; env->SetLongArrayRegion(out, 0, count, o); }
    return st;
}
FMJ(jint, impliedVolatilityHost)(JNIEnv* env, jclass, jint model, jfloatArray priceOrNull, jdouble priceScalar, jfloatArray forwardOrNull, jdouble forwardScalar,
                                 jfloatArray payoffUnitOrNull, jdouble payoffUnitScalar, jint n, jdouble maturity, jdouble strike, jint outputs, jfloatArray outColumns) {
    Pin<jfloat> pc(env, priceOrNull, JNI_ABORT); Pin<jfloat> pf(env, forwardOrNull, JNI_ABORT); Pin<jfloat> pn(env, payoffUnitOrNull, JNI_ABORT); Pin<jfloat> po(env, outColumns);
    if (!po.p || n < 1 || outputs < 1 || outputs > 7) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((priceOrNull && (!pc.p || pc.length() < n)) || (forwardOrNull && (!pf.p || pf.length() < n)) || (payoffUnitOrNull && (!pn.p || pn.length() < n))) return FMHIP_ERR_INVALID_ARGUMENT;
    const int count = (outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1);
    if ((int64_t)po.length() < (int64_t)count * n) return FMHIP_ERR_INVALID_ARGUMENT;
    float* columns[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < count; ++f) columns[f] = po.p + (int64_t)f * n;
    return fmhip_implied_volatility_host((int)model, pc.p, priceScalar, pf.p, forwardScalar, pn.p, payoffUnitScalar, (int64_t)n, maturity, strike, (int)outputs, columns);
}
// ---------------------------------------------------------------- transform option value per path: a call under an exponential-affine transform as a sum over a node table
// nodes: nNodes rows of 3 + 2·nStates doubles; states, stateScalars: nStates entries each (null where nStates is 0)
FMJ(jint, transformOption)(JNIEnv* env, jclass, jdoubleArray nodes, jint nNodes, jint nStates, jlong forward, jdouble forwardScalar, jlongArray statesOrNull, jdoubleArray stateScalarsOrNull,
                           jlong payoffUnit, jdouble payoffUnitScalar, jdouble strike, jint outputs, jlongArray out) {
    if (!out || outputs < 1 || outputs > 7 || nNodes < 1 || nNodes > FMHIP_TRANSFORM_MAX_NODES || nStates < 0 || nStates > FMHIP_TRANSFORM_MAX_STATES) return FMHIP_ERR_INVALID_ARGUMENT;
    const jsize count = (jsize)((outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1));
    if (env->GetArrayLength(out) < count) return FMHIP_ERR_INVALID_ARGUMENT;
    Pin<jdouble> pt(env, nodes, JNI_ABORT); Pin<jlong> ps(env, statesOrNull, JNI_ABORT); Pin<jdouble> pc(env, stateScalarsOrNull, JNI_ABORT);
    if (!pt.p || (int64_t)pt.length() < (int64_t)nNodes * (3 + 2 * nStates)) return FMHIP_ERR_INVALID_ARGUMENT;
    if (nStates > 0 && (!ps.p || !pc.p || ps.length() < nStates || pc.length() < nStates)) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec states[FMHIP_TRANSFORM_MAX_STATES] = { 0, 0 };
    double scalars[FMHIP_TRANSFORM_MAX_STATES] = { 0.0, 0.0 };
    for (jint k = 0; k < nStates; ++k) { states[k] = (fmhip_vec)ps.p[k]; scalars[k] = pc.p[k]; }
    fmhip_vec h[3] = { 0, 0, 0 };
    const int st = fmhip_transform_option(pt.p, (int)nNodes, (int)nStates, forward, forwardScalar, states, scalars, payoffUnit, payoffUnitScalar, strike, (int)outputs, h);
    if (st == FMHIP_OK) { jlong o[3]; for (jsize f = 0; f < count; ++f) o[f] = (jlong)h[f]; env->SetLongArrayRegion(out, 0, count, o); }
    return st;
}
FMJ(jint, transformOptionHost)(JNIEnv* env, jclass, jdoubleArray nodes, jint nNodes, jint nStates, jfloatArray forwardOrNull, jdouble forwardScalar, jfloatArray state0OrNull,
                               jfloatArray state1OrNull, jdoubleArray stateScalarsOrNull, jfloatArray payoffUnitOrNull, jdouble payoffUnitScalar, jint n, jdouble strike, jint outputs,
                               jfloatArray outColumns) {
    Pin<jdouble> pt(env, nodes, JNI_ABORT); Pin<jdouble> pc(env, stateScalarsOrNull, JNI_ABORT);
    Pin<jfloat> pf(env, forwardOrNull, JNI_ABORT); Pin<jfloat> p0(env, state0OrNull, JNI_ABORT); Pin<jfloat> p1(env, state1OrNull, JNI_ABORT); Pin<jfloat> pn(env, payoffUnitOrNull, JNI_ABORT);
    Pin<jfloat> po(env, outColumns);
    if (!po.p || n < 1 || outputs < 1 || outputs > 7 || nNodes < 1 || nNodes > FMHIP_TRANSFORM_MAX_NODES || nStates < 0 || nStates > FMHIP_TRANSFORM_MAX_STATES) return FMHIP_ERR_INVALID_ARGUMENT;
    if (!pt.p || (int64_t)pt.length() < (int64_t)nNodes * (3 + 2 * nStates) || (nStates > 0 && (!pc.p || pc.length() < nStates))) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((forwardOrNull && (!pf.p || pf.length() < n)) || (state0OrNull && (!p0.p || p0.length() < n)) || (state1OrNull && (!p1.p || p1.length() < n))
        || (payoffUnitOrNull && (!pn.p || pn.length() < n))) return FMHIP_ERR_INVALID_ARGUMENT;
    const int count = (outputs & 1) + ((outputs >> 1) & 1) + ((outputs >> 2) & 1);
    if ((int64_t)po.length() < (int64_t)count * n) return FMHIP_ERR_INVALID_ARGUMENT;
    const float* states[FMHIP_TRANSFORM_MAX_STATES] = { nStates > 0 ? p0.p : nullptr, nStates > 1 ? p1.p : nullptr };
    double scalars[FMHIP_TRANSFORM_MAX_STATES] = { 0.0, 0.0 };
    for (jint k = 0; k < nStates; ++k) scalars[k] = pc.p[k];
    float* columns[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < count; ++f) columns[f] = po.p + (int64_t)f * n;
    return fmhip_transform_option_host(pt.p, (int)nNodes, (int)nStates, pf.p, forwardScalar, states, scalars, pn.p, payoffUnitScalar, (int64_t)n, strike, (int)outputs, columns);
}
// ---------------------------------------------------------------- polynomial regression in one pass: the monomials of the states are formed in registers
// exponents: states.length (nStates) entries per term, each 0 … 6, as ints; anything outside a byte is refused here, the rest by the library
static bool poly_exponents(const jint* e, int64_t count, std::vector<uint8_t>& out) {
    if (!e || count < 0) return false;
    out.resize((size_t)count);
    for (int64_t i = 0; i < count; ++i) { if (e[i] < 0 || e[i] > 255) return false; out[(size_t)i] = (uint8_t)e[i]; }
    return true;
}
FMJ(jint, polynomialCrossMoments)(JNIEnv* env, jclass, jlongArray states, jintArray exponents, jlongArray extraX, jlongArray y, jdoubleArray sumsOut) {
    Pin<jlong> ps(env, states, JNI_ABORT); Pin<jint> pe(env, exponents, JNI_ABORT); Pin<jlong> px(env, extraX, JNI_ABORT); Pin<jlong> py(env, y, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!ps.p || !pe.p || !po.p || ps.length() < 1 || pe.length() % ps.length() != 0) return FMHIP_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> ex;
    if (!poly_exponents(pe.p, pe.length(), ex)) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nt = pe.length() / ps.length(), ne = px.p ? px.length() : 0, ny = py.p ? py.length() : 0, nx = nt + ne;
    if ((int64_t)po.length() < nx * (nx + 1) / 2 + nx * ny) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_polynomial_cross_moments((const fmhip_vec*)ps.p, ps.length(), ex.data(), (int)nt, ne ? (const fmhip_vec*)px.p : nullptr, (int)ne, ny ? (const fmhip_vec*)py.p : nullptr, (int)ny, po.p);
}
FMJ(jint, polynomialEvaluate)(JNIEnv* env, jclass, jlongArray states, jintArray exponents, jlongArray extraX, jdoubleArray coefficients, jlongArray out) {
    Pin<jlong> ps(env, states, JNI_ABORT); Pin<jint> pe(env, exponents, JNI_ABORT); Pin<jlong> px(env, extraX, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT);
    if (!ps.p || !pe.p || !pc.p || ps.length() < 1 || pe.length() % ps.length() != 0) return FMHIP_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> ex;
    if (!poly_exponents(pe.p, pe.length(), ex)) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t nt = pe.length() / ps.length(), ne = px.p ? px.length() : 0;
    if ((int64_t)pc.length() < nt + ne) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_vec h = 0;
    const int st = fmhip_polynomial_evaluate((const fmhip_vec*)ps.p, ps.length(), ex.data(), (int)nt, ne ? (const fmhip_vec*)px.p : nullptr, (int)ne, pc.p, &h);
    if (st == FMHIP_OK) set1(env, out, (jlong)h);
    return st;
}
// columns as in binnedCrossMomentsHost: nStates (nExtra, nY) columns of n floats each, one after the other; bit i of onesMask: extra i is the constant 1
static bool poly_columns(const jfloat* flat, int64_t flatLength, int64_t n, int count, int onesMask, std::vector<const float*>& out) {
    if (count < 0 || count > 64) return false;
    for (int i = 0; i < count; ++i) {
        if (i < 31 && ((onesMask >> i) & 1)) { out.push_back(nullptr); continue; }
        if (!flat || flatLength < (int64_t)(i + 1) * n) return false;
        out.push_back(flat + (int64_t)i * n);
    }
    return true;
}
FMJ(jint, polynomialCrossMomentsHost)(JNIEnv* env, jclass, jfloatArray stateColumns, jint nStates, jintArray exponents, jfloatArray extraColumns, jint nExtra, jint onesMask, jfloatArray yColumns, jint nY, jdoubleArray sumsOut) {
    Pin<jfloat> ps(env, stateColumns, JNI_ABORT); Pin<jint> pe(env, exponents, JNI_ABORT); Pin<jfloat> px(env, extraColumns, JNI_ABORT); Pin<jfloat> py(env, yColumns, JNI_ABORT); Pin<jdouble> po(env, sumsOut);
    if (!ps.p || !pe.p || !po.p || nStates < 1 || nStates > 8 || ps.length() % nStates != 0 || pe.length() % nStates != 0) return FMHIP_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> ex;
    if (!poly_exponents(pe.p, pe.length(), ex)) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = ps.length() / nStates, nt = pe.length() / nStates, nx = nt + nExtra;
    std::vector<const float*> ss, xs, ys;
    if (!poly_columns(ps.p, ps.length(), n, nStates, 0, ss) || !poly_columns(px.p, px.p ? px.length() : 0, n, nExtra, onesMask, xs) || !poly_columns(py.p, py.p ? py.length() : 0, n, nY, 0, ys)) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)po.length() < nx * (nx + 1) / 2 + nx * nY) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_polynomial_cross_moments_host(ss.data(), n, nStates, ex.data(), (int)nt, nExtra ? xs.data() : nullptr, nExtra, nY ? ys.data() : nullptr, nY, po.p);
}
FMJ(jint, polynomialEvaluateHost)(JNIEnv* env, jclass, jfloatArray stateColumns, jint nStates, jintArray exponents, jfloatArray extraColumns, jint nExtra, jint onesMask, jdoubleArray coefficients, jfloatArray out) {
    Pin<jfloat> ps(env, stateColumns, JNI_ABORT); Pin<jint> pe(env, exponents, JNI_ABORT); Pin<jfloat> px(env, extraColumns, JNI_ABORT); Pin<jdouble> pc(env, coefficients, JNI_ABORT); Pin<jfloat> po(env, out);
    if (!ps.p || !pe.p || !pc.p || !po.p || nStates < 1 || nStates > 8 || ps.length() % nStates != 0 || pe.length() % nStates != 0) return FMHIP_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> ex;
    if (!poly_exponents(pe.p, pe.length(), ex)) return FMHIP_ERR_INVALID_ARGUMENT;
    const int64_t n = ps.length() / nStates, nt = pe.length() / nStates;
    std::vector<const float*> ss, xs;
    if (!poly_columns(ps.p, ps.length(), n, nStates, 0, ss) || !poly_columns(px.p, px.p ? px.length() : 0, n, nExtra, onesMask, xs)) return FMHIP_ERR_INVALID_ARGUMENT;
    if ((int64_t)pc.length() < nt + nExtra || (int64_t)po.length() < n) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_polynomial_evaluate_host(ss.data(), n, nStates, ex.data(), (int)nt, nExtra ? xs.data() : nullptr, nExtra, pc.p, po.p);
}
FMJ(jint, reduceMomentsBatchDevice)(JNIEnv* env, jclass, jlongArray vectors, jdoubleArray shifts, jlong deviceOut) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jdouble> ps(env, shifts, JNI_ABORT);
    if (!pv.p || (ps.p && ps.length() < pv.length())) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_reduce_moments_batch_device((const fmhip_vec*)pv.p, pv.length(), ps.p, (void*)(intptr_t)deviceOut);
}
FMJ(jint, reduceMomentsBatchDevices)(JNIEnv* env, jclass, jlongArray vectors, jdoubleArray shifts, jlongArray deviceOutPerDevice) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jdouble> ps(env, shifts, JNI_ABORT); Pin<jlong> po(env, deviceOutPerDevice, JNI_ABORT);
    if (!pv.p || !po.p || (ps.p && ps.length() < pv.length())) return FMHIP_ERR_INVALID_ARGUMENT;
    std::vector<void*> out((size_t)po.length());
    for (int d = 0; d < po.length(); ++d) out[(size_t)d] = (void*)(intptr_t)po.p[d];
    return fmhip_reduce_moments_batch_devices((const fmhip_vec*)pv.p, pv.length(), ps.p, out.data(), po.length());
}
FMJ(jint, getStreamOf)(JNIEnv* env, jclass, jint shard, jlongArray stream) {
    void* s = nullptr;
    const int st = fmhip_get_stream_of(shard, &s);
    if (st == FMHIP_OK) set1(env, stream, (jlong)(intptr_t)s);
    return st;
}
FMJ(jint, expectationCollective)(JNIEnv* env, jclass, jintArray kind) {
    int k = 0;
    const int st = fmhip_expectation_collective(&k, nullptr, 0);
    if (st == FMHIP_OK && kind && env->GetArrayLength(kind) >= 1) { const jint v = k; env->SetIntArrayRegion(kind, 0, 1, &v); }
    return st;
}
FMJ(jint, reduceMomentsBatchBegin)(JNIEnv* env, jclass, jlongArray vectors, jdoubleArray shifts, jlongArray ticket) {
    Pin<jlong> pv(env, vectors, JNI_ABORT); Pin<jdouble> ps(env, shifts, JNI_ABORT);
    if (!pv.p || !ticket || env->GetArrayLength(ticket) < 1 || (ps.p && ps.length() < pv.length())) return FMHIP_ERR_INVALID_ARGUMENT;
    fmhip_ticket t = 0;
    const int st = fmhip_reduce_moments_batch_begin((const fmhip_vec*)pv.p, pv.length(), ps.p, &t);
    if (st == FMHIP_OK) { const jlong v = (jlong)t; env->SetLongArrayRegion(ticket, 0, 1, &v); }
    return st;
}
FMJ(jint, vecGiveUpValues)(JNIEnv* env, jclass, jlongArray vectors) {
    Pin<jlong> pv(env, vectors, JNI_ABORT);
    if (!pv.p) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_vec_give_up_values((const fmhip_vec*)pv.p, pv.length());
}
FMJ(jint, reduceMomentsBatchEnd)(JNIEnv* env, jclass, jlong ticket, jdoubleArray moments4PerVector, jint count) {
    Pin<jdouble> pm(env, moments4PerVector);
    if (!pm.p || count <= 0 || (int64_t)pm.length() < 4 * (int64_t)count) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_reduce_moments_batch_end((fmhip_ticket)ticket, (fmhip_moments*)pm.p, count);
}
FMJ(jint, setExpectationComm)(JNIEnv*, jclass, jint world, jint rank, jlong gatherFunction, jlong context) {
    return fmhip_set_expectation_comm(world, rank, (fmhip_gather_fn)(intptr_t)gatherFunction, (void*)(intptr_t)context);
}
FMJ(jint, expectationWorld)(JNIEnv* env, jclass, jintArray world, jintArray rank) {
    int w = 1, r = 0;
    const int st = fmhip_expectation_world(&w, &r);
    if (st == FMHIP_OK) { set1(env, world, w); set1(env, rank, r); }
    return st;
}
FMJ(jint, expectationCombine)(JNIEnv* env, jclass, jdoubleArray gathered, jint world, jint count, jdoubleArray moments4PerVector) {
    Pin<jdouble> pg(env, gathered, JNI_ABORT), pm(env, moments4PerVector);
    if (world < 1 || count < 0 || !pg.p || !pm.p || (int64_t)pg.length() < 4 * (int64_t)world * count || (int64_t)pm.length() < 4 * (int64_t)count) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_expectation_combine((const fmhip_moments*)pg.p, world, count, (fmhip_moments*)pm.p);
}

// ---------------------------------------------------------------- explicit fused programs
FMJ(jlong, programCreate)(JNIEnv* env, jclass, jintArray opcode, jintArray a, jintArray b, jintArray c, jdoubleArray scalar, jint nInputs, jintArray outValues, jintArray reduceValues) {
    std::vector<fmhip_prog_op> ops;
    if (!program_ops(env, opcode, a, b, c, scalar, ops)) return 0;
    Pin<jint> po(env, outValues, JNI_ABORT), pr(env, reduceValues, JNI_ABORT);
    fmhip_program out = 0;
    return fmhip_program_create(ops.data(), (int)ops.size(), nInputs, (const int32_t*)po.p, po.length(), (const int32_t*)pr.p, pr.length(), &out) == FMHIP_OK ? (jlong)out : 0;
}
FMJ(jint, programRelease)(JNIEnv*, jclass, jlong p) { return fmhip_program_release(p); }
FMJ(jint, programLaunchCount)(JNIEnv* env, jclass, jlong p, jintArray launches) { int n = 0; const int st = fmhip_program_launch_count(p, &n); if (st == FMHIP_OK) set1(env, launches, n); return st; }
FMJ(jint, programShape)(JNIEnv* env, jclass, jlong p, jintArray inputsOutputsReductions3) {
    int shape[3] = { 0, 0, 0 };
    const int st = fmhip_program_shape(p, &shape[0], &shape[1], &shape[2]);
    if (st == FMHIP_OK && inputsOutputsReductions3 && env->GetArrayLength(inputsOutputsReductions3) >= 3) { const jint v[3] = { shape[0], shape[1], shape[2] }; env->SetIntArrayRegion(inputsOutputsReductions3, 0, 3, v); }
    return st;
}
namespace {
// the arrays of programRun / programRunInto against the program's shape: batch x inputs handles in, batch x outputs handles,
// one shift per reduction, 4 doubles per row and reduction
bool run_arrays_fit(jlong p, jint batch, const Pin<jlong>& in, const Pin<jlong>& out, const Pin<jdouble>& shift, const Pin<jdouble>& moments) {
    int n_in = 0, n_out = 0, n_red = 0;
    if (batch <= 0 || fmhip_program_shape(p, &n_in, &n_out, &n_red) != FMHIP_OK) return false;
    const int64_t b = batch;
    return in.p && (int64_t)in.length() >= b * n_in && (n_out == 0 || (out.p && (int64_t)out.length() >= b * n_out)) &&
           (!shift.p || shift.length() >= n_red) && (!moments.p || (int64_t)moments.length() >= 4 * b * n_red);
}
}
FMJ(jint, programRun)(JNIEnv* env, jclass, jlong p, jint batch, jlongArray inputs, jlongArray outputs, jdoubleArray reduceShift, jdoubleArray moments4, jlong deviceMoments) {
    Pin<jlong> pi(env, inputs, JNI_ABORT), po(env, outputs); Pin<jdouble> ps(env, reduceShift, JNI_ABORT), pm(env, moments4);
    if (!run_arrays_fit(p, batch, pi, po, ps, pm)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_program_run(p, batch, (const fmhip_vec*)pi.p, (fmhip_vec*)po.p, ps.p, (fmhip_moments*)pm.p, (void*)(intptr_t)deviceMoments);
}
FMJ(jint, programRunInto)(JNIEnv* env, jclass, jlong p, jint batch, jlongArray inputs, jlongArray outputs, jdoubleArray reduceShift, jdoubleArray moments4, jlong deviceMoments) {
    Pin<jlong> pi(env, inputs, JNI_ABORT), po(env, outputs, JNI_ABORT); Pin<jdouble> ps(env, reduceShift, JNI_ABORT), pm(env, moments4);
    if (!run_arrays_fit(p, batch, pi, po, ps, pm)) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_program_run_into(p, batch, (const fmhip_vec*)pi.p, (const fmhip_vec*)po.p, ps.p, (fmhip_moments*)pm.p, (void*)(intptr_t)deviceMoments);
}

// ---------------------------------------------------------------- execution tiers
FMJ(jint, setJit)(JNIEnv* env, jclass, jint mode, jintArray previous) { int prev = 0; const int st = fmhip_set_jit(mode, &prev); if (st == FMHIP_OK) set1(env, previous, prev); return st; }
FMJ(jint, jitWait)(JNIEnv*, jclass) { return fmhip_jit_wait(); }
FMJ(jint, jitStats)(JNIEnv* env, jclass, jlongArray compiledFailedPendingDiskHits, jdoubleArray compileSeconds) {
    int64_t compiled = 0, failed = 0, pending = 0, disk = 0; double seconds = 0.0;
    const int st = fmhip_jit_stats(&compiled, &failed, &pending, &seconds, &disk);
    if (st == FMHIP_OK) {
        if (compiledFailedPendingDiskHits && env->GetArrayLength(compiledFailedPendingDiskHits) >= 4) { const jlong v[4] = { (jlong)compiled, (jlong)failed, (jlong)pending, (jlong)disk }; env->SetLongArrayRegion(compiledFailedPendingDiskHits, 0, 4, v); }
        if (compileSeconds && env->GetArrayLength(compileSeconds) >= 1) env->SetDoubleArrayRegion(compileSeconds, 0, 1, &seconds);
    }
    return st;
}
FMJ(jint, programTier)(JNIEnv* env, jclass, jlong p, jintArray tierAndVgprs) {
    int tier = 0, vgprs = 0;
    const int st = fmhip_program_tier(p, &tier, &vgprs);
    if (st == FMHIP_OK && tierAndVgprs && env->GetArrayLength(tierAndVgprs) >= 2) { const jint v[2] = { tier, vgprs }; env->SetIntArrayRegion(tierAndVgprs, 0, 2, v); }
    return st;
}
FMJ(jstring, programSource)(JNIEnv* env, jclass, jintArray opcode, jintArray a, jintArray b, jintArray c, jdoubleArray scalar, jint nInputs, jintArray outValues, jintArray reduceValues) {
    std::vector<fmhip_prog_op> ops;
    if (!program_ops(env, opcode, a, b, c, scalar, ops)) return nullptr;
    std::vector<int32_t> outs, reds;
    { Pin<jint> po(env, outValues, JNI_ABORT), pr(env, reduceValues, JNI_ABORT); outs.assign(po.p, po.p + po.length()); reds.assign(pr.p, pr.p + pr.length()); }
    int64_t needed = 0;
    if (fmhip_program_source(ops.data(), (int)ops.size(), nInputs, outs.data(), (int)outs.size(), reds.data(), (int)reds.size(), nullptr, 0, &needed) != FMHIP_OK) return nullptr;
    std::string text((size_t)needed + 1, '\0');
    if (fmhip_program_source(ops.data(), (int)ops.size(), nInputs, outs.data(), (int)outs.size(), reds.data(), (int)reds.size(), &text[0], needed + 1, &needed) != FMHIP_OK) return nullptr;
    return env->NewStringUTF(text.c_str());
}

// ---------------------------------------------------------------- Brownian increments
FMJ(jint, bmGenerate)(JNIEnv* env, jclass, jlong seed, jint nSteps, jint nFactors, jlong nPaths, jlong pathOffset, jdoubleArray dt, jlongArray outHandles) {
    Pin<jdouble> pd(env, dt, JNI_ABORT); Pin<jlong> po(env, outHandles);
    if (nSteps <= 0 || nFactors <= 0 || !po.p || !pd.p || (int64_t)po.length() < (int64_t)nSteps * nFactors || pd.length() < nSteps) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_bm_generate(seed, nSteps, nFactors, nPaths, pathOffset, pd.p, (fmhip_vec*)po.p);
}
FMJ(jint, mersenneIncrements)(JNIEnv* env, jclass, jint seed, jint nSteps, jint nFactors, jlong nPaths, jdoubleArray dt, jdoubleArray hostOut) {
    Pin<jdouble> pd(env, dt, JNI_ABORT), po(env, hostOut);
    if (nSteps <= 0 || nFactors <= 0 || nPaths < 0 || !po.p || !pd.p || (int64_t)po.length() < (int64_t)nSteps * nFactors * nPaths || pd.length() < nSteps) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_mersenne_increments(seed, nSteps, nFactors, nPaths, pd.p, po.p);
}
FMJ(jint, bmGenerateMersenne)(JNIEnv* env, jclass, jint seed, jint nSteps, jint nFactors, jlong nPaths, jdoubleArray dt, jlongArray outHandles) {
    Pin<jdouble> pd(env, dt, JNI_ABORT); Pin<jlong> po(env, outHandles);
    if (nSteps <= 0 || nFactors <= 0 || !po.p || !pd.p || (int64_t)po.length() < (int64_t)nSteps * nFactors || pd.length() < nSteps) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_bm_generate_mersenne(seed, nSteps, nFactors, nPaths, pd.p, (fmhip_vec*)po.p);
}
FMJ(jint, bmGenerateMersenneDevice)(JNIEnv* env, jclass, jint seed, jint nSteps, jint nFactors, jlong nPaths, jlong pathOffset, jdoubleArray dt, jlongArray outHandles) {
    Pin<jdouble> pd(env, dt, JNI_ABORT); Pin<jlong> po(env, outHandles);
    if (nSteps <= 0 || nFactors <= 0 || !po.p || !pd.p || (int64_t)po.length() < (int64_t)nSteps * nFactors || pd.length() < nSteps) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_bm_generate_mersenne_device(seed, nSteps, nFactors, nPaths, pathOffset, pd.p, (fmhip_vec*)po.p);
}
FMJ(jint, incrementsHost)(JNIEnv* env, jclass, jint seed, jint nSteps, jint nFactors, jlong nPaths, jintArray kinds, jdoubleArray a, jdoubleArray b, jdoubleArray hostOut) {
    Pin<jint> pk(env, kinds, JNI_ABORT); Pin<jdouble> pa(env, a, JNI_ABORT), pb(env, b, JNI_ABORT), po(env, hostOut);
    const int64_t laws = (int64_t)nSteps * nFactors;
    if (nSteps <= 0 || nFactors <= 0 || nPaths < 0 || !pk.p || !pa.p || !pb.p || !po.p || pk.length() < laws || pa.length() < laws || pb.length() < laws || (int64_t)po.length() < laws * nPaths) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_increments_host(seed, nSteps, nFactors, nPaths, (const int32_t*)pk.p, pa.p, pb.p, po.p);
}
FMJ(jint, incrementsGenerateDevice)(JNIEnv* env, jclass, jint seed, jint nSteps, jint nFactors, jlong nPaths, jlong pathOffset, jintArray kinds, jdoubleArray a, jdoubleArray b, jlongArray outHandles) {
    Pin<jint> pk(env, kinds, JNI_ABORT); Pin<jdouble> pa(env, a, JNI_ABORT), pb(env, b, JNI_ABORT); Pin<jlong> po(env, outHandles);
    const int64_t laws = (int64_t)nSteps * nFactors;
    if (nSteps <= 0 || nFactors <= 0 || !pk.p || !pa.p || !pb.p || !po.p || pk.length() < laws || pa.length() < laws || pb.length() < laws || (int64_t)po.length() < laws) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_increments_generate_device(seed, nSteps, nFactors, nPaths, pathOffset, (const int32_t*)pk.p, pa.p, pb.p, (fmhip_vec*)po.p);
}
FMJ(jint, sobolPointsHost)(JNIEnv* env, jclass, jint nDims, jlong firstIndex, jlong count, jint seed, jint randomize, jdoubleArray uOut) {
    Pin<jdouble> po(env, uOut);
    if (nDims <= 0 || count < 0 || !po.p || (int64_t)po.length() < (int64_t)nDims * count) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_sobol_points_host(nDims, firstIndex, count, seed, randomize, po.p);
}
FMJ(jint, sobolIncrementsHost)(JNIEnv* env, jclass, jint seed, jint randomize, jint construction, jint nSteps, jint nFactors, jlong nPaths, jlong pathOffset, jdoubleArray dt, jdoubleArray hostOut) {
    Pin<jdouble> pd(env, dt, JNI_ABORT), po(env, hostOut);
    if (nSteps <= 0 || nFactors <= 0 || nPaths < 0 || !pd.p || !po.p || pd.length() < nSteps || (int64_t)po.length() < (int64_t)nSteps * nFactors * nPaths) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_sobol_increments_host(seed, randomize, construction, nSteps, nFactors, nPaths, pathOffset, pd.p, po.p);
}
FMJ(jint, bmGenerateSobolDevice)(JNIEnv* env, jclass, jint seed, jint randomize, jint construction, jint nSteps, jint nFactors, jlong nPaths, jlong pathOffset, jdoubleArray dt, jlongArray outHandles) {
    Pin<jdouble> pd(env, dt, JNI_ABORT); Pin<jlong> po(env, outHandles);
    if (nSteps <= 0 || nFactors <= 0 || !po.p || !pd.p || (int64_t)po.length() < (int64_t)nSteps * nFactors || pd.length() < nSteps) return FMHIP_ERR_INVALID_ARGUMENT;
    return fmhip_bm_generate_sobol_device(seed, randomize, construction, nSteps, nFactors, nPaths, pathOffset, pd.p, (fmhip_vec*)po.p);
}
FMJ(jdouble, inverseNormalCdf)(JNIEnv*, jclass, jdouble p) { return fmhip_inverse_normal_cdf(p); }

// ---------------------------------------------------------------- pool
FMJ(jint, poolClean)(JNIEnv*, jclass) { return fmhip_pool_clean(); }
FMJ(jint, poolPurge)(JNIEnv*, jclass) { return fmhip_pool_purge(); }
FMJ(jint, poolStats)(JNIEnv* env, jclass, jlongArray stats10) {
    fmhip_pool_stats_t s;
    const int st = fmhip_pool_stats(&s);
    static_assert(sizeof(fmhip_pool_stats_t) == 10 * sizeof(int64_t), "pool statistics travel as 10 longs");
    if (st == FMHIP_OK && stats10 && env->GetArrayLength(stats10) >= 10) env->SetLongArrayRegion(stats10, 0, 10, (const jlong*)&s);
    return st;
}

// ---------------------------------------------------------------- measurement
FMJ(jint, profileEnable)(JNIEnv*, jclass, jint enabled) { return fmhip_profile_enable(enabled); }
FMJ(jint, trafficStats)(JNIEnv* env, jclass, jlongArray algorithmicBytesAndSpecialisedLaunches) {
    int64_t bytes = 0, launches = 0;
    const int st = fmhip_traffic_stats(&bytes, &launches);
    if (st == FMHIP_OK && algorithmicBytesAndSpecialisedLaunches && env->GetArrayLength(algorithmicBytesAndSpecialisedLaunches) >= 2) { const jlong v[2] = { (jlong)bytes, (jlong)launches }; env->SetLongArrayRegion(algorithmicBytesAndSpecialisedLaunches, 0, 2, v); }
    return st;
}
FMJ(jint, engineStats)(JNIEnv* env, jclass, jlongArray stats18) {
    fmhip_engine_stats_t s;
    const int st = fmhip_engine_stats(&s);
    static_assert(sizeof(fmhip_engine_stats_t) == 18 * sizeof(int64_t), "engine statistics travel as 18 longs");
    if (st == FMHIP_OK && stats18) { const jsize len = env->GetArrayLength(stats18); env->SetLongArrayRegion(stats18, 0, len < 18 ? len : 18, (const jlong*)&s); }
    return st;
}
FMJ(jint, profileRead)(JNIEnv* env, jclass, jdoubleArray kernelMsTotal, jlongArray launches) {
    double ms = 0.0; int64_t n = 0;
    const int st = fmhip_profile_read(&ms, &n);
    if (st == FMHIP_OK) { if (kernelMsTotal && env->GetArrayLength(kernelMsTotal) >= 1) env->SetDoubleArrayRegion(kernelMsTotal, 0, 1, &ms); set1(env, launches, (jlong)n); }
    return st;
}
