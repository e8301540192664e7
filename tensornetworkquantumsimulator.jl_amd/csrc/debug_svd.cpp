// debug_svd.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the SVD and Cholesky kernels (kernels_svd.hip, kernels_chol.hip, svd_batch's tall route).
#include "debug_util.hpp"

using namespace tnqs;

extern "C" int tnqs_dbg_jacobi(int dtype, int m, int n, void* A, void* V, int* sweeps) {
    return guard([&] {
        need_gpu();
        if (m < 1 || n < 1 || m > 256 || n > 256) throw Err(TNQS_ERR_INVALID, "dbg_jacobi: 1 <= m, n <= 256");
        const size_t esz = esz_of(dtype);
        DBuf dA((size_t)m * n * esz), dV((size_t)n * n * esz), dS(4); DevItems<JacobiItem> dI(1);
        dA.up(A, (size_t)m * n * esz);
        by_dtype(dtype, [&](auto t) { launch_identity<decltype(t)>(nullptr, dV.p, n); });
        // same residency policy as the engine: A+V in LDS, else A in LDS with V recovered, else global memory
        const size_t lim = 160 * 1024 - 2048;
        size_t lds_av = jacobi_lds_bytes(m, n, true, esz), lds_a = jacobi_lds_bytes(m, n, false, esz);
        const char* fg = std::getenv("TNQS_DBG_NOV_GLOBAL");      // the engine's combination for matrices beyond the LDS: global-memory kernel, V recovered
        const bool force_global_nov = fg && fg[0] == '1';
        const char* ft = std::getenv("TNQS_DBG_THETA_SVD");       // the engine's theta route: A only in LDS, V recovered from the unrotated copy
        const bool theta_route = ft && ft[0] == '1' && dtype == TNQS_C64 && lds_a <= lim;
        const bool nov = force_global_nov || theta_route || (lds_av > lim && lds_a <= lim);
        DBuf dA0((size_t)m * n * esz);
        if (nov) dA0.up(A, (size_t)m * n * esz);
        dI.up(JacobiItem{dA.p, nov ? nullptr : dV.p, m, n, (int*)dS.p});
        size_t lds = force_global_nov ? 0 : (nov ? lds_a : (lds_av <= lim ? lds_av : 0));
        by_dtype(dtype, [&](auto t) { launch_jacobi<decltype(t)>(nullptr, dI.get(), 1, 60, lds, std::max(m, n)); });
        if (nov) {
            DevItems<RecoverItem> dRv(1); dRv.up(RecoverItem{dA0.p, dA.p, dV.p, m, n, n});
            if (dtype == TNQS_C64) launch_recover_v_mfma(nullptr, dRv.get(), 1, n); else launch_recover_v<double>(nullptr, dRv.get(), 1, n);
            HIPCHK(hipDeviceSynchronize());
        }
        HIPCHK(hipDeviceSynchronize());
        dA.down(A, (size_t)m * n * esz); dV.down(V, (size_t)n * n * esz);
        if (sweeps) dS.down(sweeps, 4);
    });
}

// theta_svd_pre_kernel on one ComplexF32 factor A (m x n) of theta = A Q^T, Q (nq x n, complex128, orthonormal columns): A := U Sigma, V (nq x n) := conj(Q) U_L.
// reps > 0: additionally time `reps` launches on `copies` device-resident copies of A (one workgroup each) with HIP events -> *ms = average per launch
extern "C" int tnqs_dbg_theta_svd_pre(int m, int n, int nq, void* A, const void* Q, void* V, int* sweeps, int copies, int reps, double* ms, double* phase_us, int cap) {
    return guard([&] {
        need_gpu();
        if (!Q) nq = n;                                 // no Q: theta itself is factorised, V is n x n
        if (!theta_svd_pre_covers(m, n) || nq < n || nq > m) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_pre: 2 <= n <= 64, n <= nq <= m <= 128");
        if (copies < 1) copies = 1;
        const size_t ab = (size_t)m * n * 8, vb = (size_t)nq * n * 8;
        DBuf dA(ab * copies), dA0(ab), dQ((size_t)nq * n * 16), dV(vb * copies), dS(4 * (size_t)copies), dInfo(32); DevItems<JacobiItem> dI(copies); DBuf dT(64);
        dA0.up(A, ab); if (Q) dQ.up(Q, (size_t)nq * n * 16);
        const int info[8] = {m, nq, 0, 0, 0, 0, 0, Q ? n : 0};      // theta_dims with d1 = d2 = 1: m rows, nq columns of theta, n columns of the factor (0: theta itself)
        dInfo.up(info, 32);
        std::vector<JacobiItem> its(copies);
        for (int c = 0; c < copies; ++c) {
            JacobiItem it{}; it.A = (char*)dA.p + ab * c; it.V = (c == 0 && phase_us) ? dT.p : nullptr; it.m = m; it.n = nq; it.sweeps_out = (int*)dS.p + c; it.dyn = (const int*)dInfo.p; it.dm = 1; it.dn = 1; it.nhint = n;
            it.QB = Q ? dQ.p : nullptr; it.Vout = (char*)dV.p + vb * c; it.pre = 0 /* the dimensions given decide, whatever the size */; it.cap = cap; its[c] = it;
        }
        dI.up(its);
        auto reset = [&]() { for (int c = 0; c < copies; ++c) HIPCHK(hipMemcpyAsync((char*)dA.p + ab * c, dA0.p, ab, hipMemcpyDeviceToDevice, nullptr)); };
        reset();
        launch_theta_svd_pre(nullptr, dI.get(), copies, 60, m, n);
        HIPCHK(hipDeviceSynchronize());
        dA.down(A, ab); dV.down(V, vb);
        if (sweeps) dS.down(sweeps, 4);
        if (phase_us) {      // constant-rate clock (100 MHz) at the seven phase boundaries of workgroup 0 -> six durations in us
            unsigned long long t[8]; dT.down(t, 64);
            for (int k = 0; k < 6; ++k) phase_us[k] = (double)(t[k + 1] - t[k]) * 0.01;
        }
        if (reps > 0 && ms) {
            hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
            double tot = 0;
            for (int r = 0; r < reps; ++r) {
                reset();
                HIPCHK(hipEventRecord(e0, nullptr));
                launch_theta_svd_pre(nullptr, dI.get(), copies, 60, m, n);
                HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1));
                float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1)); tot += t;
            }
            *ms = tot / reps;
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        }
    });
}
// the plain LDS-resident Jacobi on the same factor, timed the same way (what the preconditioned kernel replaces)
extern "C" int tnqs_dbg_time_jacobi_f32(int m, int n, const void* A, int copies, int reps, double* ms, int* sweeps) {
    return guard([&] {
        need_gpu();
        if (copies < 1) copies = 1;
        const size_t ab = (size_t)m * n * 8;
        DBuf dA(ab * copies), dA0(ab), dS(4 * (size_t)copies); DevItems<JacobiItem> dI(copies);
        dA0.up(A, ab);
        std::vector<JacobiItem> its(copies);
        for (int c = 0; c < copies; ++c) { JacobiItem it{}; it.A = (char*)dA.p + ab * c; it.m = m; it.n = n; it.sweeps_out = (int*)dS.p + c; its[c] = it; }
        dI.up(its);
        hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        double tot = 0;
        for (int r = 0; r < reps + 1; ++r) {
            for (int c = 0; c < copies; ++c) HIPCHK(hipMemcpyAsync((char*)dA.p + ab * c, dA0.p, ab, hipMemcpyDeviceToDevice, nullptr));
            HIPCHK(hipEventRecord(e0, nullptr));
            launch_jacobi<float>(nullptr, dI.get(), copies, 60, jacobi_lds_bytes(m, n, false, 8), std::max(m, n), n);
            HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1));
            float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1)); if (r > 0) tot += t;
        }
        if (ms) *ms = tot / std::max(1, reps);
        if (sweeps) dS.down(sweeps, 4);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    });
}

// Cholesky kernels on one Hermitian n x n complex128 matrix: L (lower), W = (L^-1)^dagger, *fail; n <= 96: chol_kernel, else packed
extern "C" int tnqs_dbg_chol(int n, const void* G, void* Lout, void* Wout, int* fail, double tau) {
    return guard([&] {
        need_gpu();
        if (n < 1 || n > 128) throw Err(TNQS_ERR_INVALID, "dbg_chol: 1 <= n <= 128");
        const size_t b = (size_t)n * n * 16;
        DBuf dG(b), dL(b), dW(b), dF(4); DevItems<CholItem> dI(1);
        dG.up(G, b); HIPCHK(hipMemset(dF.p, 0, 4)); HIPCHK(hipMemset(dW.p, 0, b));
        dI.up(CholItem{dG.p, dL.p, dW.p, n, (int*)dF.p, tau, 0.0});
        if (n <= 96) launch_chol(nullptr, dI.get(), 1, n); else launch_chol_packed(nullptr, dI.get(), 1, n);
        HIPCHK(hipDeviceSynchronize());
        dL.down(Lout, b); dW.down(Wout, b); dF.down(fail, 4);
    });
}

// svd_batch's tall route (svd_tall: Cholesky-QR, Jacobi on R, A J, polish where the pivot collapsed) on nitems ComplexF32 matrices A_i (m[i] x n[i],
// one after the other): A_i <- U Sigma; chol_fail[i]: the packed Cholesky refused a pivot; polished[i]: the polishing sweeps ran on the item;
// sweeps[i]: the sweeps of the Jacobi on R
extern "C" int tnqs_dbg_svd_tall(int nitems, const int* m, const int* n, void* A, int* chol_fail, int* polished, int* sweeps) {
    return guard([&] {
        need_gpu();
        if (nitems < 1 || !m || !n || !A) throw Err(TNQS_ERR_INVALID, "dbg_svd_tall: bad arguments");
        for (int i = 0; i < nitems; ++i)
            if (n[i] < 2 || n[i] > 128 || m[i] < n[i] || m[i] > 512) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_svd_tall: 2 <= n <= 128, n <= m <= 512");
        std::vector<size_t> off; cat_offsets(nitems, off, [&](int i) { return (size_t)m[i] * n[i]; });
        int dev = 0; HIPCHK(hipGetDevice(&dev));
        std::unique_ptr<State> s(state_create(1, 0, nullptr, nullptr, nullptr, TNQS_C64, dev));
        {
            // every matrix starts at a multiple of 256 bytes, as the engine's theta slots do (an odd m n would leave the next one at 8 bytes only); the gaps keep
            // their 0xff filling, checked below
            Slots sA; for (int i = 0; i < nitems; ++i) sA.add((size_t)m[i] * n[i] * 8);
            sA.alloc(); put_all(sA, A); sA.up();
            DBuf dF(sizeof(int) * nitems), dS(sizeof(int) * nitems), dW(sizeof(int) * nitems);
            HIPCHK(hipMemset(dS.p, 0, sizeof(int) * nitems)); HIPCHK(hipMemset(dW.p, 0xff, sizeof(int) * nitems));      // polish sweeps: -1 = not run
            std::vector<JacobiItem> tall(nitems);
            for (int i = 0; i < nitems; ++i) { JacobiItem j{}; j.A = sA.at(i); j.m = m[i]; j.n = n[i]; j.sweeps_out = (int*)dS.p + i; tall[i] = j; }
            svd_tall(s.get(), tall, (int*)dF.p, (int*)dW.p);
            HIPCHK(hipStreamSynchronize(s->stream));
            sA.down("the matrices");
            for (int i = 0; i < nitems; ++i) sA.get(i, (char*)A + off[i] * 8);
            std::vector<int> f(nitems), w(nitems);
            dF.down(f.data(), sizeof(int) * nitems); dW.down(w.data(), sizeof(int) * nitems);
            if (sweeps) dS.down(sweeps, sizeof(int) * nitems);
            for (int i = 0; i < nitems; ++i) { if (chol_fail) chol_fail[i] = f[i]; if (polished) polished[i] = w[i] >= 0; }
        }
    });
}
