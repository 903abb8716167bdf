    /* oracle/thompson_column_part2.inc -- continuation of th_column(): mp_thompson.f90:2012-2844 */

    /* ---- :2015-2110 do not deplete more than exists ---- */
    for (k = kts; k <= kte; ++k) {
        sump = (float)(pri_inu[k] + pri_ide[k] + prs_ide[k] + prs_sde[k] + prg_gde[k]);
        rate_max = (qv[k] - qvsi[k]) * odts * 0.999f;
        if ((sump > eps && sump > rate_max) || (sump < -eps && sump < rate_max)) {
            ratio = rate_max / sump;
            pri_inu[k] *= ratio; pri_ide[k] *= ratio; pni_ide[k] *= ratio; prs_ide[k] *= ratio; prs_sde[k] *= ratio; prg_gde[k] *= ratio;
        }
        sump = (float)(-prr_wau[k] - pri_wfz[k] - prr_rcw[k] - prs_scw[k] - prg_scw[k] - prg_gcw[k]);
        rate_max = -rc[k] * odts;
        if (sump < rate_max && L_qc[k]) {
            ratio = rate_max / sump;
            prr_wau[k] *= ratio; pri_wfz[k] *= ratio; prr_rcw[k] *= ratio; prs_scw[k] *= ratio; prg_scw[k] *= ratio; prg_gcw[k] *= ratio;
        }
        sump = (float)(pri_ide[k] - prs_iau[k] - prs_sci[k] - pri_rci[k]);
        rate_max = -ri[k] * odts;
        if (sump < rate_max && L_qi[k]) {
            ratio = rate_max / sump;
            pri_ide[k] *= ratio; prs_iau[k] *= ratio; prs_sci[k] *= ratio; pri_rci[k] *= ratio;
        }
        sump = (float)(-prg_rfz[k] - pri_rfz[k] - prr_rci[k] + prr_rcs[k] + prr_rcg[k]);
        rate_max = -rr[k] * odts;
        if (sump < rate_max && L_qr[k]) {
            ratio = rate_max / sump;
            prg_rfz[k] *= ratio; pri_rfz[k] *= ratio; prr_rci[k] *= ratio; prr_rcs[k] *= ratio; prr_rcg[k] *= ratio;
        }
        sump = (float)(prs_sde[k] - prs_ihm[k] - prr_sml[k] + prs_rcs[k]);
        rate_max = -rs[k] * odts;
        if (sump < rate_max && L_qs[k]) {
            ratio = rate_max / sump;
            prs_sde[k] *= ratio; prs_ihm[k] *= ratio; prr_sml[k] *= ratio; prs_rcs[k] *= ratio;
        }
        sump = (float)(prg_gde[k] - prg_ihm[k] - prr_gml[k] + prg_rcg[k]);
        rate_max = -rg[k] * odts;
        if (sump < rate_max && L_qg[k]) {
            ratio = rate_max / sump;
            prg_gde[k] *= ratio; prg_ihm[k] *= ratio; prr_gml[k] *= ratio; prg_rcg[k] *= ratio;
        }
        pri_ihm[k] = prs_ihm[k] + prg_ihm[k];
        ratio = (float)fmin(fabs(prr_rcg[k]), fabs(prg_rcg[k]));
        prr_rcg[k] = ratio * copysignf(1.0f, (float)prr_rcg[k]);
        prg_rcg[k] = -prr_rcg[k];
        if (temp[k] > T_0) {
            ratio = (float)fmin(fabs(prr_rcs[k]), fabs(prs_rcs[k]));
            prr_rcs[k] = ratio * copysignf(1.0f, (float)prr_rcs[k]);
            prs_rcs[k] = -prr_rcs[k];
        }
    }

    /* ---- :2116-2236 tendencies ---- */
    for (k = kts; k <= kte; ++k) {
        orho = 1.f / rho[k];
        lfus2 = lsub - lvap[k];
        qvten[k] = (float)(qvten[k] + (-pri_inu[k] - pri_ide[k] - prs_ide[k] - prs_sde[k] - prg_gde[k]) * orho);
        qcten[k] = (float)(qcten[k] + (-prr_wau[k] - pri_wfz[k] - prr_rcw[k] - prs_scw[k] - prg_scw[k] - prg_gcw[k]) * orho);
        qiten[k] = (float)(qiten[k] + (pri_inu[k] + pri_ihm[k] + pri_wfz[k] + pri_rfz[k] + pri_ide[k]
                                       - prs_iau[k] - prs_sci[k] - pri_rci[k]) * orho);
        niten[k] = (float)(niten[k] + (pni_inu[k] + pni_ihm[k] + pni_wfz[k] + pni_rfz[k] + pni_ide[k]
                                       - pni_iau[k] - pni_sci[k] - pni_rci[k]) * orho);
        xri = fmaxf(R1, (qi1d[k] + qiten[k] * dtsave) * rho[k]);
        xni = fmaxf(R2, (ni1d[k] + niten[k] * dtsave) * rho[k]);
        if (xri > R1) {
            lami = M_powf(am_i * cig[1] * TH.oig1 * xni / xri, TH.obmi);
            ilami = 1. / lami;
            xDi = (float)((double)(bm_i + mu_i + 1.f) * ilami);
            if (xDi < 20.E-6f) {
                lami = cie[1] / 20.E-6f;
                xni = (float)fmin(250.e3, (double)(cig[0] * TH.oig2 * xri / am_i) * (lami * lami * lami));
                niten[k] = (xni - ni1d[k] * rho[k]) * odts * orho;
            } else if (xDi > 300.E-6f) {
                lami = cie[1] / 300.E-6f;
                xni = (float)((double)(cig[0] * TH.oig2 * xri / am_i) * (lami * lami * lami));
                niten[k] = (xni - ni1d[k] * rho[k]) * odts * orho;
            }
        } else niten[k] = -ni1d[k] * odts;
        xni = fmaxf(0.f, (ni1d[k] + niten[k] * dtsave) * rho[k]);
        if (xni > 250.E3f) niten[k] = (250.E3f - ni1d[k] * rho[k]) * odts * orho;

        qrten[k] = (float)(qrten[k] + (prr_wau[k] + prr_rcw[k] + prr_sml[k] + prr_gml[k] + prr_rcs[k] + prr_rcg[k]
                                       - prg_rfz[k] - pri_rfz[k] - prr_rci[k]) * orho);
        nrten[k] = (float)(nrten[k] + (pnr_wau[k] + pnr_sml[k] + pnr_gml[k]
                                       - (pnr_rfz[k] + pnr_rcr[k] + pnr_rcg[k] + pnr_rcs[k] + pnr_rci[k])) * orho);
        xrr = fmaxf(R1, (qr1d[k] + qrten[k] * dtsave) * rho[k]);
        xnr = fmaxf(R2, (nr1d[k] + nrten[k] * dtsave) * rho[k]);
        if (xrr > R1) {
            lamr = M_powf(am_r * crg[2] * TH.org2 * xnr / xrr, TH.obmr);
            mvd_r[k] = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r[k] > 2.5E-3f) {
                mvd_r[k] = 2.5E-3f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r[k];
                xnr = (float)((double)(crg[1] * TH.org3 * xrr) * (lamr * lamr * lamr) / (double)am_r);
                nrten[k] = (xnr - nr1d[k] * rho[k]) * odts * orho;
            } else if (mvd_r[k] < D0r * 0.75f) {
                mvd_r[k] = D0r * 0.75f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r[k];
                xnr = (float)((double)(crg[1] * TH.org3 * xrr) * (lamr * lamr * lamr) / (double)am_r);
                nrten[k] = (xnr - nr1d[k] * rho[k]) * odts * orho;
            }
        } else { qrten[k] = -qr1d[k] * odts; nrten[k] = -nr1d[k] * odts; }

        qsten[k] = (float)(qsten[k] + (prs_iau[k] + prs_sde[k] + prs_sci[k] + prs_scw[k] + prs_rcs[k] + prs_ide[k]
                                       - prs_ihm[k] - prr_sml[k]) * orho);
        qgten[k] = (float)(qgten[k] + (prg_scw[k] + prg_rfz[k] + prg_gde[k] + prg_rcg[k] + prg_gcw[k] + prg_rci[k]
                                       + prg_rcs[k] - prg_ihm[k] - prr_gml[k]) * orho);
        if (temp[k] < T_0) {
            tten[k] = (float)(tten[k] + ((double)(lsub * ocp[k]) * (pri_inu[k] + pri_ide[k] + prs_ide[k] + prs_sde[k] + prg_gde[k])
                              + (double)(lfus2 * ocp[k]) * (pri_wfz[k] + pri_rfz[k] + prg_rfz[k] + prs_scw[k] + prg_scw[k] + prg_gcw[k]
                                                             + prg_rcs[k] + prs_rcs[k] + prr_rci[k] + prg_rcg[k])) * orho * 1);
        } else {
            tten[k] = (float)(tten[k] + ((double)(TH_lfus * ocp[k]) * (-prr_sml[k] - prr_gml[k] - prr_rcg[k] - prr_rcs[k])
                              + (double)(lsub * ocp[k]) * (prs_sde[k] + prg_gde[k])) * orho * 1);
        }
    }

    /* ---- :2241-2318 update to TAU+1 ---- */
    for (k = kts; k <= kte; ++k) {
        temp[k] = t1d[k] + dt * tten[k];
        otemp = 1.f / temp[k];
        tempc = temp[k] - 273.15f;
        qv[k] = fmaxf(1.E-10f, qv1d[k] + dt * qvten[k]);
        rho[k] = 0.622f * pres[k] / (TH_RR2 * temp[k] * (qv[k] + 0.622f));
        rhof[k] = sqrtf(TH_rho_not / rho[k]);
        rhof2[k] = sqrtf(rhof[k]);
        qvs[k] = rslf(pres[k], temp[k]);
        ssatw[k] = qv[k] / qvs[k] - 1.f;
        if (fabsf(ssatw[k]) < eps) ssatw[k] = 0.0f;
        diffu[k] = 2.11E-5f * M_powf(temp[k] / 273.15f, 1.94f) * (101325.f / pres[k]);
        if (tempc >= 0.0f) visco[k] = (1.718f + 0.0049f * tempc) * 1.0E-5f;
        else visco[k] = (1.718f + 0.0049f * tempc - 1.2E-5f * tempc * tempc) * 1.0E-5f;
        vsc2[k] = sqrtf(rho[k] / visco[k]);
        lvap[k] = lvap0 + (2106.0f - 4218.0f) * tempc;
        tcond[k] = (5.69f + 0.0168f * tempc) * 1.0E-5f * 418.936f;
        ocp[k] = 1.f / (TH_Cp2 * (1.f + 0.887f * qv[k]));
        lvt2[k] = lvap[k] * lvap[k] * ocp[k] * oRv * otemp * otemp;

        if ((qc1d[k] + qcten[k] * dt) > R1) { rc[k] = (qc1d[k] + qcten[k] * dt) * rho[k]; L_qc[k] = 1; }
        else { rc[k] = R1; L_qc[k] = 0; }
        if ((qi1d[k] + qiten[k] * dt) > R1) {
            ri[k] = (qi1d[k] + qiten[k] * dt) * rho[k];
            ni[k] = fmaxf(R2, (ni1d[k] + niten[k] * dt) * rho[k]);
            L_qi[k] = 1;
        } else { ri[k] = R1; ni[k] = R2; L_qi[k] = 0; }
        if ((qr1d[k] + qrten[k] * dt) > R1) {
            rr[k] = (qr1d[k] + qrten[k] * dt) * rho[k];
            nr[k] = fmaxf(R2, (nr1d[k] + nrten[k] * dt) * rho[k]);
            L_qr[k] = 1;
            lamr = M_powf(am_r * crg[2] * TH.org2 * nr[k] / rr[k], TH.obmr);
            mvd_r[k] = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r[k] > 2.5E-3f) {
                mvd_r[k] = 2.5E-3f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r[k];
                nr[k] = (float)((double)(crg[1] * TH.org3 * rr[k]) * (lamr * lamr * lamr) / (double)am_r);
            } else if (mvd_r[k] < D0r * 0.75f) {
                mvd_r[k] = D0r * 0.75f;
                lamr = (3.0f + mu_r + 0.672f) / mvd_r[k];
                nr[k] = (float)((double)(crg[1] * TH.org3 * rr[k]) * (lamr * lamr * lamr) / (double)am_r);
            }
        } else { rr[k] = R1; nr[k] = R2; L_qr[k] = 0; }
        if ((qs1d[k] + qsten[k] * dt) > R1) { rs[k] = (qs1d[k] + qsten[k] * dt) * rho[k]; L_qs[k] = 1; }
        else { rs[k] = R1; L_qs[k] = 0; }
        if ((qg1d[k] + qgten[k] * dt) > R1) { rg[k] = (qg1d[k] + qgten[k] * dt) * rho[k]; L_qg[k] = 1; }
        else { rg[k] = R1; L_qg[k] = 0; }
    }

    /* ---- :2325-2374 snow moments again (smob, smo2, smoc, smod) ---- */
    for (k = kts; k <= kte; ++k) {
        if (!L_qs[k]) continue;
        tc0 = fminf(-0.1f, temp[k] - 273.15f);
        smob[k] = rs[k] * TH.oams;
        if (TH_bm_s > (2.0f - 1.e-3f) && TH_bm_s < (2.0f + 1.e-3f)) smo2[k] = smob[k];
        else {
            loga_ = snow_poly_f(sa, tc0, TH_bm_s); a_ = M_powf(10.0f, loga_); b_ = snow_poly_f(sb, tc0, TH_bm_s);
            smo2[k] = M_powf(smob[k] / a_, 1.f / b_);
        }
        loga_ = snow_poly_f(sa, tc0, TH.cse[0]); a_ = M_powf(10.0f, loga_); b_ = snow_poly_f(sb, tc0, TH.cse[0]);
        smoc[k] = a_ * M_powf(smo2[k], b_);
        loga_ = snow_poly_f(sa, tc0, TH.cse[13]); a_ = M_powf(10.0f, loga_); b_ = snow_poly_f(sb, tc0, TH.cse[13]);
        smod[k] = a_ * M_powf(smo2[k], b_);
    }

    /* ---- :2379-2396 graupel intercept/slope again ---- */
    N0_min = TH_gonv_max;
    for (k = kte; k >= kts; --k) {
        if (temp[k] < 270.65f && L_qr[k] && mvd_r[k] > 100.E-6f) xslw1 = 4.01f + M_log10f(mvd_r[k]);
        else xslw1 = 0.01f;
        ygra1 = 4.31f + M_log10f(fmaxf(5.E-5f, rg[k]));
        zans1 = 3.1f + (100.f / (300.f * xslw1 * ygra1 / (10.f / xslw1 + 1.f + 0.25f * ygra1) + 30.f + 10.f * ygra1));
        N0_exp = M_powf(10.f, zans1);
        N0_exp = fmax((double)TH_gonv_min, fmin(N0_exp, (double)TH_gonv_max));
        N0_min = fmin(N0_exp, N0_min);
        N0_exp = N0_min;
        lam_exp = pow(N0_exp * am_g * cgg[0] / rg[k], (double)TH.oge1);
        lamg = lam_exp * M_powf(cgg[2] * TH.ogg2 * TH.ogg1, TH.obmg);
        ilamg[k] = 1. / lamg;
        N0_g[k] = N0_exp / (cgg[1] * lam_exp) * pow(lamg, (double)cge[1]);
    }
    /* ---- :2403-2408 rain ---- */
    for (k = kte; k >= kts; --k) {
        lamr = M_powf(am_r * crg[2] * TH.org2 * nr[k] / rr[k], TH.obmr);
        ilamr[k] = 1. / lamr;
        mvd_r[k] = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
        N0_r[k] = (double)(nr[k] * TH.org2) * pow(lamr, (double)cre[1]);
    }

    /* ---- :2414-2440 cloud water condensation / evaporation (3 Newton-Raphson iterations) ---- */
    for (k = kts; k <= kte; ++k) {
        if ((ssatw[k] > eps) || (ssatw[k] < -eps && L_qc[k])) {
            clap = (qv[k] - qvs[k]) / (1.f + lvt2[k] * qvs[k]);
            for (n = 1; n <= 3; ++n) {
                fcd = qvs[k] * M_expf(lvt2[k] * clap) - qv[k] + clap;
                dfcd = qvs[k] * lvt2[k] * M_expf(lvt2[k] * clap) + 1.f;
                clap = clap - fcd / dfcd;
            }
            xrc = rc[k] + clap;
            if (xrc > 0.0f) prw_vcd[k] = clap * odt;
            else prw_vcd[k] = -rc[k] / rho[k] * odts;
            qcten[k] = (float)(qcten[k] + prw_vcd[k]);
            qvten[k] = (float)(qvten[k] - prw_vcd[k]);
            tten[k] = (float)(tten[k] + (double)(lvap[k] * ocp[k]) * prw_vcd[k] * 1);
            rc[k] = fmaxf(R1, (qc1d[k] + dt * qcten[k]) * rho[k]);
            qv[k] = fmaxf(1.E-10f, qv1d[k] + dt * qvten[k]);
            temp[k] = t1d[k] + dt * tten[k];
            rho[k] = 0.622f * pres[k] / (TH_RR2 * temp[k] * (qv[k] + 0.622f));
            qvs[k] = rslf(pres[k], temp[k]);
            ssatw[k] = qv[k] / qvs[k] - 1.f;
        }
    }

    /* ---- :2446-2505 rain evaporation ---- */
    for (k = kts; k <= kte; ++k) {
        if ((ssatw[k] < -eps) && L_qr[k] && (!(prw_vcd[k] > 0.))) {
            tempc = temp[k] - 273.15f;
            otemp = 1.f / temp[k];
            rhof[k] = sqrtf(TH_rho_not / rho[k]);
            rhof2[k] = sqrtf(rhof[k]);
            diffu[k] = 2.11E-5f * M_powf(temp[k] / 273.15f, 1.94f) * (101325.f / pres[k]);
            if (tempc >= 0.0f) visco[k] = (1.718f + 0.0049f * tempc) * 1.0E-5f;
            else visco[k] = (1.718f + 0.0049f * tempc - 1.2E-5f * tempc * tempc) * 1.0E-5f;
            vsc2[k] = sqrtf(rho[k] / visco[k]);
            lvap[k] = lvap0 + (2106.0f - 4218.0f) * tempc;
            tcond[k] = (5.69f + 0.0168f * tempc) * 1.0E-5f * 418.936f;
            ocp[k] = 1.f / (TH_Cp2 * (1.f + 0.887f * qv[k]));
            rvs = rho[k] * qvs[k];
            rvs_p = rvs * otemp * (lvap[k] * otemp * oRv - 1.f);
            rvs_pp = rvs * (otemp * (lvap[k] * otemp * oRv - 1.f) * otemp * (lvap[k] * otemp * oRv - 1.f)
                            + (-2.f * lvap[k] * otemp * otemp * otemp * oRv) + otemp * otemp);
            gamsc = lvap[k] * diffu[k] / tcond[k] * rvs_p;
            alphsc = 0.5f * (gamsc / (1.f + gamsc)) * (gamsc / (1.f + gamsc)) * rvs_pp / rvs_p * rvs / rvs_p;
            alphsc = fmaxf(1.E-9f, alphsc);
            xsat = fminf(-1.E-9f, ssatw[k]);
            t1_evap = 2.f * PI2 * (1.0f - alphsc * xsat + 2.f * alphsc * alphsc * xsat * xsat
                                   - 5.f * alphsc * alphsc * alphsc * xsat * xsat * xsat) / (1.f + gamsc);
            lamr = 1. / ilamr[k];
            if (qv[k] / qvs[k] < 0.95f && rr[k] / rho[k] <= 1.E-8f) {
                prv_rev[k] = rr[k] / rho[k] * odts;
            } else {
                prv_rev[k] = (double)(t1_evap * diffu[k] * (-ssatw[k])) * N0_r[k] * (double)rvs
                             * ((double)TH.t1_qr_ev * pow(ilamr[k], (double)cre[9])
                                + (double)(TH.t2_qr_ev * vsc2[k] * rhof2[k]) * pow(lamr + (double)(0.5f * fv_r), -(double)cre[10]));
                rate_max = fminf((rr[k] / rho[k] * odts), (qvs[k] - qv[k]) * odts);
                prv_rev[k] = fmin((double)rate_max, prv_rev[k] / (double)rho[k]);
            }
            pnr_rev[k] = fmin((double)(nr[k] * 0.99f / rho[k] * odts), prv_rev[k] * (double)nr[k] / (double)rr[k]);
            qrten[k] = (float)(qrten[k] - prv_rev[k]);
            qvten[k] = (float)(qvten[k] + prv_rev[k]);
            nrten[k] = (float)(nrten[k] - pnr_rev[k]);
            tten[k] = (float)(tten[k] - (double)(lvap[k] * ocp[k]) * prv_rev[k] * 1);
            rr[k] = fmaxf(R1, (qr1d[k] + dt * qrten[k]) * rho[k]);
            qv[k] = fmaxf(1.E-10f, qv1d[k] + dt * qvten[k]);
            nr[k] = fmaxf(R2, (nr1d[k] + dt * nrten[k]) * rho[k]);
            temp[k] = t1d[k] + dt * tten[k];
            rho[k] = 0.622f * pres[k] / (TH_RR2 * temp[k] * (qv[k] + 0.622f));
        }
    }

    /* ---- :2515-2650 terminal fall speeds and sub-step counts ---- */
    nstep = 0;
    for (n = 0; n < 4; ++n) { onstep[n] = 1.0f; ksed1[n] = 0; }
    for (k = kte + 1; k >= kts; --k) { vtrk[k] = 0.f; vtnrk[k] = 0.f; vtik[k] = 0.f; vtnik[k] = 0.f; vtsk[k] = 0.f; vtgk[k] = 0.f; }
    for (k = kte; k >= kts; --k) {
        vtr = 0.f;
        rhof[k] = sqrtf(TH_rho_not / rho[k]);
        if (rr[k] > R1) {
            lamr = M_powf(am_r * crg[2] * TH.org2 * nr[k] / rr[k], TH.obmr);
            vtr = (float)((double)(rhof[k] * TH_av_r * crg[5] * TH.org3) * pow(lamr, (double)cre[2]) * pow(lamr + (double)fv_r, -(double)cre[5]));
            vtrk[k] = vtr;
            vtr = (float)((double)(rhof[k] * TH_av_r * crg[6] / crg[11]) * pow(lamr, (double)cre[11]) * pow(lamr + (double)fv_r, -(double)cre[6]));
            vtnrk[k] = vtr;
        } else { vtrk[k] = vtrk[k + 1]; vtnrk[k] = vtnrk[k + 1]; }
        if (fmaxf(vtrk[k], vtnrk[k]) > 1.E-3f) {
            ksed1[0] = imax(ksed1[0], k);
            delta_tp = dzq[k] / (fmaxf(vtrk[k], vtnrk[k]));
            nstep = imax(nstep, (int)(dt / delta_tp + 1.f));
        }
    }
    if (ksed1[0] == kte) ksed1[0] = kte - 1;
    if (nstep > 0) onstep[0] = 1.f / (float)nstep;

    nstep = 0;
    for (k = kte; k >= kts; --k) {
        vti = 0.f;
        if (ri[k] > R1) {
            lami = M_powf(am_i * cig[1] * TH.oig1 * ni[k] / ri[k], TH.obmi);
            ilami = 1. / lami;
            vti = (float)((double)(rhof[k] * TH.av_i * cig[2] * TH.oig2) * ilami);
            vtik[k] = vti;
            vti = (float)((double)(rhof[k] * TH.av_i * cig[5] / cig[6]) * ilami);
            vtnik[k] = vti;
        } else { vtik[k] = vtik[k + 1]; vtnik[k] = vtnik[k + 1]; }
        if (vtik[k] > 1.E-3f) {
            ksed1[1] = imax(ksed1[1], k);
            delta_tp = dzq[k] / vtik[k];
            nstep = imax(nstep, (int)(dt / delta_tp + 1.f));
        }
    }
    if (ksed1[1] == kte) ksed1[1] = kte - 1;
    if (nstep > 0) onstep[1] = 1.f / (float)nstep;

    nstep = 0;
    for (k = kte; k >= kts; --k) {
        vts = 0.f;
        if (rs[k] > R1) {
            xDs = smoc[k] / smob[k];
            Mrat = 1.f / xDs;
            ils1 = 1.f / (Mrat * TH_Lam0 + TH.fv_s);
            ils2 = 1.f / (Mrat * TH_Lam1 + TH.fv_s);
            t1_vts = TH_Kap0 * TH.csg[3] * M_powf(ils1, TH.cse[3]);
            t2_vts = TH_Kap1 * M_powf(Mrat, TH_mu_s) * TH.csg[9] * M_powf(ils2, TH.cse[9]);
            ils1 = 1.f / (Mrat * TH_Lam0);
            ils2 = 1.f / (Mrat * TH_Lam1);
            t3_vts = TH_Kap0 * TH.csg[0] * M_powf(ils1, TH.cse[0]);
            t4_vts = TH_Kap1 * M_powf(Mrat, TH_mu_s) * TH.csg[6] * M_powf(ils2, TH.cse[6]);
            vts = rhof[k] * TH.av_s * (t1_vts + t2_vts) / (t3_vts + t4_vts);
            if (temp[k] > T_0) vtsk[k] = fmaxf(vts * vts_boost[k], vtrk[k]);
            else vtsk[k] = vts * vts_boost[k];
        } else vtsk[k] = vtsk[k + 1];
        if (vtsk[k] > 1.E-3f) {
            ksed1[2] = imax(ksed1[2], k);
            delta_tp = dzq[k] / vtsk[k];
            nstep = imax(nstep, (int)(dt / delta_tp + 1.f));
        }
    }
    if (ksed1[2] == kte) ksed1[2] = kte - 1;
    if (nstep > 0) onstep[2] = 1.f / (float)nstep;

    nstep = 0;
    for (k = kte; k >= kts; --k) {
        vtg = 0.f;
        if (rg[k] > R1) {
            vtg = (float)((double)(rhof[k] * av_g * cgg[5] * TH.ogg3) * pow(ilamg[k], (double)bv_g));
            if (temp[k] > T_0) vtgk[k] = fmaxf(vtg, vtrk[k]); else vtgk[k] = vtg;
        } else vtgk[k] = vtgk[k + 1];
        if (vtgk[k] > 1.E-3f) {
            ksed1[3] = imax(ksed1[3], k);
            delta_tp = dzq[k] / vtgk[k];
            nstep = imax(nstep, (int)(dt / delta_tp + 1.f));
        }
    }
    if (ksed1[3] == kte) ksed1[3] = kte - 1;
    if (nstep > 0) onstep[3] = 1.f / (float)nstep;
    if (g_th_diag) {
        int hr[KMAX], hi[KMAX], hs[KMAX], hg[KMAX];
        for (k = kts; k <= kte; ++k) { hr[k] = rr[k] > R1; hi[k] = ri[k] > R1; hs[k] = rs[k] > R1; hg[k] = rg[k] > R1; }
        for (n = 0; n < 4; ++n) th_diag_col[n] = (int)lroundf(1.f / onstep[n]);
        th_diag_species(0, hr, vtrk, kts, kte); th_diag_species(1, hi, vtik, kts, kte);
        th_diag_species(2, hs, vtsk, kts, kte); th_diag_species(3, hg, vtgk, kts, kte);
    }

    /* ---- :2660-2770 sedimentation ---- */
    nstep = (int)lroundf(1.f / onstep[0]);
    for (n = 1; n <= nstep; ++n) {
        for (k = kte; k >= kts; --k) { sed_r[k] = vtrk[k] * rr[k]; sed_n[k] = vtnrk[k] * nr[k]; }
        k = kte;
        odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
        qrten[k] = qrten[k] - sed_r[k] * odzq * onstep[0] * orho;
        nrten[k] = nrten[k] - sed_n[k] * odzq * onstep[0] * orho;
        rr[k] = fmaxf(R1, rr[k] - sed_r[k] * odzq * dt * onstep[0]);
        nr[k] = fmaxf(R2, nr[k] - sed_n[k] * odzq * dt * onstep[0]);
        for (k = ksed1[0]; k >= kts; --k) {
            odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
            qrten[k] = qrten[k] + (sed_r[k + 1] - sed_r[k]) * odzq * onstep[0] * orho;
            nrten[k] = nrten[k] + (sed_n[k + 1] - sed_n[k]) * odzq * onstep[0] * orho;
            rr[k] = fmaxf(R1, rr[k] + (sed_r[k + 1] - sed_r[k]) * odzq * dt * onstep[0]);
            nr[k] = fmaxf(R2, nr[k] + (sed_n[k + 1] - sed_n[k]) * odzq * dt * onstep[0]);
        }
        if (rr[kts] > R1 * 10.f) *pptrain = *pptrain + sed_r[kts] * dt * onstep[0];
    }
    nstep = (int)lroundf(1.f / onstep[1]);
    for (n = 1; n <= nstep; ++n) {
        for (k = kte; k >= kts; --k) { sed_i[k] = vtik[k] * ri[k]; sed_n[k] = vtnik[k] * ni[k]; }
        k = kte;
        odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
        qiten[k] = qiten[k] - sed_i[k] * odzq * onstep[1] * orho;
        niten[k] = niten[k] - sed_n[k] * odzq * onstep[1] * orho;
        ri[k] = fmaxf(R1, ri[k] - sed_i[k] * odzq * dt * onstep[1]);
        ni[k] = fmaxf(R2, ni[k] - sed_n[k] * odzq * dt * onstep[1]);
        for (k = ksed1[1]; k >= kts; --k) {
            odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
            qiten[k] = qiten[k] + (sed_i[k + 1] - sed_i[k]) * odzq * onstep[1] * orho;
            niten[k] = niten[k] + (sed_n[k + 1] - sed_n[k]) * odzq * onstep[1] * orho;
            ri[k] = fmaxf(R1, ri[k] + (sed_i[k + 1] - sed_i[k]) * odzq * dt * onstep[1]);
            ni[k] = fmaxf(R2, ni[k] + (sed_n[k + 1] - sed_n[k]) * odzq * dt * onstep[1]);
        }
        if (ri[kts] > R1 * 10.f) *pptice = *pptice + sed_i[kts] * dt * onstep[1];
    }
    nstep = (int)lroundf(1.f / onstep[2]);
    for (n = 1; n <= nstep; ++n) {
        for (k = kte; k >= kts; --k) sed_s[k] = vtsk[k] * rs[k];
        k = kte;
        odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
        qsten[k] = qsten[k] - sed_s[k] * odzq * onstep[2] * orho;
        rs[k] = fmaxf(R1, rs[k] - sed_s[k] * odzq * dt * onstep[2]);
        for (k = ksed1[2]; k >= kts; --k) {
            odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
            qsten[k] = qsten[k] + (sed_s[k + 1] - sed_s[k]) * odzq * onstep[2] * orho;
            rs[k] = fmaxf(R1, rs[k] + (sed_s[k + 1] - sed_s[k]) * odzq * dt * onstep[2]);
        }
        if (rs[kts] > R1 * 10.f) *pptsnow = *pptsnow + sed_s[kts] * dt * onstep[2];
    }
    nstep = (int)lroundf(1.f / onstep[3]);
    for (n = 1; n <= nstep; ++n) {
        for (k = kte; k >= kts; --k) sed_g[k] = vtgk[k] * rg[k];
        k = kte;
        odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
        qgten[k] = qgten[k] - sed_g[k] * odzq * onstep[3] * orho;
        rg[k] = fmaxf(R1, rg[k] - sed_g[k] * odzq * dt * onstep[3]);
        for (k = ksed1[3]; k >= kts; --k) {
            odzq = 1.f / dzq[k]; orho = 1.f / rho[k];
            qgten[k] = qgten[k] + (sed_g[k + 1] - sed_g[k]) * odzq * onstep[3] * orho;
            rg[k] = fmaxf(R1, rg[k] + (sed_g[k + 1] - sed_g[k]) * odzq * dt * onstep[3]);
        }
        if (rg[kts] > R1 * 10.f) *pptgraul = *pptgraul + sed_g[kts] * dt * onstep[3];
    }

    /* ---- :2777-2794 instant melt / freeze ---- */
    for (k = kts; k <= kte; ++k) {
        xri = fmaxf(0.0f, qi1d[k] + qiten[k] * dt);
        if ((temp[k] > T_0) && (xri > 0.0f)) {
            qcten[k] = qcten[k] + xri * odt;
            qiten[k] = qiten[k] - xri * odt;
            niten[k] = -ni1d[k] * odt;
            tten[k] = tten[k] - TH_lfus * ocp[k] * xri * odt * 1;
        }
        xrc = fmaxf(0.0f, qc1d[k] + qcten[k] * dt);
        if ((temp[k] < HGFR) && (xrc > 0.0f)) {
            lfus2 = lsub - lvap[k];
            qiten[k] = qiten[k] + xrc * odt;
            niten[k] = niten[k] + xrc / xm0i * odt;
            qcten[k] = qcten[k] - xrc * odt;
            tten[k] = tten[k] + lfus2 * ocp[k] * xrc * odt * 1;
        }
    }

    /* ---- :2800-2842 apply tendencies ---- */
    for (k = kts; k <= kte; ++k) {
        t1d[k] = t1d[k] + tten[k] * dt;
        qv1d[k] = fmaxf(1.E-10f, qv1d[k] + qvten[k] * dt);
        qc1d[k] = qc1d[k] + qcten[k] * dt;
        if (qc1d[k] <= R1) qc1d[k] = 0.0f;
        qi1d[k] = qi1d[k] + qiten[k] * dt;
        ni1d[k] = fmaxf(R2 / rho[k], ni1d[k] + niten[k] * dt);
        if (qi1d[k] <= R1) { qi1d[k] = 0.0f; ni1d[k] = 0.0f; }
        else {
            lami = M_powf(am_i * cig[1] * TH.oig1 * ni1d[k] / qi1d[k], TH.obmi);
            ilami = 1. / lami;
            xDi = (float)((double)(bm_i + mu_i + 1.f) * ilami);
            if (xDi < 20.E-6f) lami = cie[1] / 20.E-6f;
            else if (xDi > 300.E-6f) lami = cie[1] / 300.E-6f;
            ni1d[k] = (float)fmin((double)(cig[0] * TH.oig2 * qi1d[k] / am_i) * (lami * lami * lami), 250.e3 / (double)rho[k]);
        }
        qr1d[k] = qr1d[k] + qrten[k] * dt;
        nr1d[k] = fmaxf(R2 / rho[k], nr1d[k] + nrten[k] * dt);
        if (qr1d[k] <= R1) { qr1d[k] = 0.0f; nr1d[k] = 0.0f; }
        else {
            lamr = M_powf(am_r * crg[2] * TH.org2 * nr1d[k] / qr1d[k], TH.obmr);
            mvd_r[k] = (float)((double)(3.0f + mu_r + 0.672f) / lamr);
            if (mvd_r[k] > 2.5E-3f) mvd_r[k] = 2.5E-3f;
            else if (mvd_r[k] < D0r * 0.75f) mvd_r[k] = D0r * 0.75f;
            lamr = (3.0f + mu_r + 0.672f) / mvd_r[k];
            nr1d[k] = (float)((double)(crg[1] * TH.org3 * qr1d[k]) * (lamr * lamr * lamr) / (double)am_r);
        }
        qs1d[k] = qs1d[k] + qsten[k] * dt;
        if (qs1d[k] <= R1) qs1d[k] = 0.0f;
        qg1d[k] = qg1d[k] + qgten[k] * dt;
        if (qg1d[k] <= R1) qg1d[k] = 0.0f;
    }
    (void)rgvm; (void)sed_s; (void)sed_g; (void)sed_i; (void)xnc; (void)sump;
