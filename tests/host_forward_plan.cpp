// Prints the ForwardPlan (gator_amd/csrc/forward_plan.h) of every case given on the command line, one line per case.  A case is a
// comma-separated list of name=value: the planner's inputs (J, n_cu, B, entry, bf16, joints, pin) and any field of FusedOptions; what a
// case does not name keeps its default.  Built by tests/test_host_forward_plan.py as plain C++17: the header needs no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "forward_plan.h"

using namespace gator;

struct PlanInput { int J = 17, n_cu = 256, B = 1; PlanEntry entry = PlanEntry::FORWARD; bool bf16 = false, joints = false; int pin = -1; };

static bool set_field(FusedOptions& o, PlanInput& in, const std::string& k, int v) {
#define OPT(name) if (k == #name) { o.name = v; return true; }
    OPT(gat_x3) OPT(gat8) OPT(gat8_h4) OPT(gat8_lobyte) OPT(gat8_tail) OPT(gat_tiled_h4) OPT(gat_tiled) OPT(gat_tiled_min_batch)
    OPT(mdr_x3) OPT(up_x3) OPT(mdr_persist) OPT(mdr_persist_chunk) OPT(mdr_persist_grid) OPT(mdr_head_partials)
    OPT(c3_mdr) OPT(c3_encoder) OPT(c3_up_w1) OPT(c3_up_bf16) OPT(mdr_stamps)
#undef OPT
    if (k == "J") in.J = v; else if (k == "n_cu") in.n_cu = v; else if (k == "B") in.B = v; else if (k == "bf16") in.bf16 = v;
    else if (k == "joints") in.joints = v; else if (k == "pin") in.pin = v;
    else if (k == "entry") in.entry = v == 1 ? PlanEntry::GAT : v == 2 ? PlanEntry::MDR : PlanEntry::FORWARD;
    else return false;
    return true;
}

int main(int argc, char** argv) {
    static const char* const sample[] = {"none", "k_gat", "k_gat8"}, * const ctr[] = {"nobody", "k_mdr_joint", "k_gat_joint", "k_gat8"},
                     * const head[] = {"finish", "head<512,true>", "head<512,false>"}, * const up[] = {"none", "fp32", "x3", "x2", "bf16"};
    for (int i = 1; i < argc; ++i) {
        FusedOptions o;
        PlanInput in;
        std::string s = argv[i];
        for (size_t at = 0; at < s.size();) {
            const size_t end = s.find(',', at) == std::string::npos ? s.size() : s.find(',', at), eq = s.find('=', at);
            if (eq == std::string::npos || eq > end || !set_field(o, in, s.substr(at, eq - at), atoi(s.c_str() + eq + 1))) {
                fprintf(stderr, "bad case '%s'\n", argv[i]);
                return 2;
            }
            at = end + 1;
        }
        ForwardPlan p, again;
        const char* why = plan_forward(o, in.J, in.n_cu, in.B, in.entry, in.bf16, in.joints, in.pin, &p);
        if (why) { printf("error=%s\n", why); continue; }
        if (plan_forward(o, in.J, in.n_cu, in.B, in.entry, in.bf16, in.joints, in.pin, &again) || !(again == p)) { fprintf(stderr, "plan of '%s' is not equal to itself\n", argv[i]); return 3; }
        printf("n_tiled=%d sample=%s k_gat8=%d,%d,%d,%d,%d k_gat=%d,%d k_gat_tiled=%d,%d,%d enc16=%d fused_tail=%d n_tail=%d ctr_zero=%s "
               "xa=%d persist=%d grid=%d nch=%d base=%d rem=%d head=%s up=%s joints=%d w1=%d\n",
               p.n_tiled, sample[(int)p.sample], p.gat8.h4, p.gat8.lr, p.gat8.h2, p.gat8.lb, p.gat8.tail, p.gat.x3k, p.gat.tail, p.tiled.J, p.tiled.h4,
               p.tiled.h2, p.enc16, p.fused_tail, p.n_tail, ctr[(int)p.ctr_zero], p.xa, p.persist, p.grid, p.chunks.nch, p.chunks.base, p.chunks.rem,
               head[(int)p.head], up[(int)p.up.form], p.up.with_joints, p.up.w1);
    }
    return 0;
}
