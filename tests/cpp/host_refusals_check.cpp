// Stand-alone check of the host layers' refusals that need no device: every public solve, select and rollout entry
// point of both modes with a null context, with a struct of the wrong struct_size, and with each table's flag set
// without its table.  Prints one line per call ("<call> [<case>]: <code> <message>"); the lines are the contract, so
// two builds of the host files are compared by diffing what this prints.  Meant to be linked against srb_capi.cpp,
// srb12_capi.cpp and srb_ll_capi.cpp compiled with -fsanitize=address,undefined (host side) plus the product's device
// objects: none of these refusals reaches a HIP call, so it runs without a GPU (`make hostcheck`).
#include <cstdio>
#include <functional>
#include <string>
#include <vector>
#include "srbnmpc.h"

namespace {

template <class T> T sized()
{
    T x{};
    x.struct_size = (int)sizeof(T);
    return x;
}

// one case: the structs every entry point is called with (a null pointer: that struct is left out)
struct Case {
    std::string name;
    srb_batch b = sized<srb_batch>();
    srb12_batch b12 = sized<srb12_batch>();
    srb_sim sim = sized<srb_sim>();
    srb12_sim sim12 = sized<srb12_sim>();
    srb12_plans pl = sized<srb12_plans>();
    srb_moving mv = sized<srb_moving>();
    srb_sizes sz = sized<srb_sizes>();
    srb_agent_sizes ag = sized<srb_agent_sizes>();
    bool with_mv = true, with_sz = true, with_ag = true, with_pl = true;
};

int failures = 0;

void report(const std::string &call, const std::string &cs, int rc)
{
    std::printf("%s [%s]: %d %s\n", call.c_str(), cs.c_str(), rc, rc ? srb_last_error() : "");
    if (rc == SRB_OK) failures++;          // every call here is one that the library refuses
}

void run_case(Case &k)
{
    static double goal[4];                 // never read: the refusals come before any launch
    k.sim.goal = goal;
    k.sim12.goal = goal;
    const srb_moving *mv = k.with_mv ? &k.mv : nullptr;
    const srb_sizes *sz = k.with_sz ? &k.sz : nullptr;
    const srb_agent_sizes *ag = k.with_ag ? &k.ag : nullptr;
    const srb12_plans *pl = k.with_pl ? &k.pl : nullptr;
    srb_ctx *c = nullptr;
    srb12_ctx *c12 = nullptr;
    const std::vector<std::pair<const char *, std::function<int()>>> calls = {
        // LIP mode: host-buffer solves, device solves, selects, rollouts
        {"srb_solve_batch", [&] { return srb_solve_batch(c, 1, &k.b); }},
        {"srb_solve_qp", [&] { return srb_solve_qp(c, 1, &k.b); }},
        {"srb_solve_batch_moving", [&] { return srb_solve_batch_moving(c, 1, &k.b, mv); }},
        {"srb_solve_batch_sized", [&] { return srb_solve_batch_sized(c, 1, &k.b, mv, sz); }},
        {"srb_solve_batch_agents", [&] { return srb_solve_batch_agents(c, 1, &k.b, mv, sz, ag); }},
        {"srb_solve_batch_device", [&] { return srb_solve_batch_device(c, 1, &k.b, nullptr); }},
        {"srb_solve_batch_moving_device", [&] { return srb_solve_batch_moving_device(c, 1, &k.b, mv, nullptr); }},
        {"srb_solve_batch_sized_device", [&] { return srb_solve_batch_sized_device(c, 1, &k.b, mv, sz, nullptr); }},
        {"srb_solve_batch_agents_device", [&] { return srb_solve_batch_agents_device(c, 1, &k.b, mv, sz, ag, nullptr); }},
        {"srb_select_device", [&] { return srb_select_device(c, 1, &k.b, 3, nullptr); }},
        {"srb_select_moving_device", [&] { return srb_select_moving_device(c, 1, &k.b, mv, 3, nullptr); }},
        {"srb_select_sized_device", [&] { return srb_select_sized_device(c, 1, &k.b, mv, sz, 3, nullptr); }},
        {"srb_select_agents_device", [&] { return srb_select_agents_device(c, 1, &k.b, mv, sz, ag, 3, nullptr); }},
        {"srb_select_agents_device tables=0", [&] { return srb_select_agents_device(c, 1, &k.b, mv, sz, ag, 0, nullptr); }},
        {"srb_sim_metrics_agents_device", [&] { return srb_sim_metrics_agents_device(c, 1, &k.sim, sz, ag, 0, nullptr); }},
        {"srb_rollout_device", [&] { return srb_rollout_device(c, 1, &k.b, &k.sim, 1, nullptr); }},
        {"srb_rollout_moving_device", [&] { return srb_rollout_moving_device(c, 1, &k.b, &k.sim, mv, 1, nullptr); }},
        {"srb_rollout_sized_device", [&] { return srb_rollout_sized_device(c, 1, &k.b, &k.sim, mv, sz, 1, nullptr); }},
        {"srb_rollout_agents_device", [&] { return srb_rollout_agents_device(c, 1, &k.b, &k.sim, mv, sz, ag, 1, nullptr); }},
        {"srb_rollout_plant_device", [&] { return srb_rollout_plant_device(c, 1, &k.b, &k.sim, mv, sz, ag, nullptr, 1, nullptr); }},
        {"srb_rollout_link_device", [&] { return srb_rollout_link_device(c, 1, &k.b, &k.sim, mv, sz, ag, nullptr, nullptr, 1, nullptr); }},
        // SRB-12 mode likewise (it has no select entry point: the solve selects)
        {"srb12_solve_batch", [&] { return srb12_solve_batch(c12, 1, &k.b12); }},
        {"srb12_solve_batch_plans", [&] { return srb12_solve_batch_plans(c12, 1, &k.b12, pl); }},
        {"srb12_solve_batch_moving", [&] { return srb12_solve_batch_moving(c12, 1, &k.b12, pl, mv); }},
        {"srb12_solve_batch_sized", [&] { return srb12_solve_batch_sized(c12, 1, &k.b12, pl, mv, sz); }},
        {"srb12_solve_batch_agents", [&] { return srb12_solve_batch_agents(c12, 1, &k.b12, pl, mv, sz, ag); }},
        {"srb12_solve_batch_device", [&] { return srb12_solve_batch_device(c12, 1, &k.b12, nullptr); }},
        {"srb12_solve_batch_plans_device", [&] { return srb12_solve_batch_plans_device(c12, 1, &k.b12, pl, nullptr); }},
        {"srb12_solve_batch_moving_device", [&] { return srb12_solve_batch_moving_device(c12, 1, &k.b12, pl, mv, nullptr); }},
        {"srb12_solve_batch_sized_device", [&] { return srb12_solve_batch_sized_device(c12, 1, &k.b12, pl, mv, sz, nullptr); }},
        {"srb12_solve_batch_agents_device", [&] { return srb12_solve_batch_agents_device(c12, 1, &k.b12, pl, mv, sz, ag, nullptr); }},
        {"srb12_solve_batch_link_device", [&] { return srb12_solve_batch_link_device(c12, 1, &k.b12, pl, mv, sz, ag, nullptr, nullptr); }},
        {"srb12_sim_metrics_agents_device", [&] { return srb12_sim_metrics_agents_device(c12, 1, &k.sim12, sz, ag, 0, nullptr); }},
        {"srb12_rollout_device", [&] { return srb12_rollout_device(c12, 1, &k.b12, &k.sim12, 1, nullptr); }},
        {"srb12_rollout_plans_device", [&] { return srb12_rollout_plans_device(c12, 1, &k.b12, &k.sim12, pl, 1, nullptr); }},
        {"srb12_rollout_moving_device", [&] { return srb12_rollout_moving_device(c12, 1, &k.b12, &k.sim12, pl, mv, 1, nullptr); }},
        {"srb12_rollout_sized_device", [&] { return srb12_rollout_sized_device(c12, 1, &k.b12, &k.sim12, pl, mv, sz, 1, nullptr); }},
        {"srb12_rollout_agents_device", [&] { return srb12_rollout_agents_device(c12, 1, &k.b12, &k.sim12, pl, mv, sz, ag, 1, nullptr); }},
        {"srb12_rollout_plant_device", [&] { return srb12_rollout_plant_device(c12, 1, &k.b12, &k.sim12, pl, mv, sz, ag, nullptr, 1, nullptr); }},
        {"srb12_rollout_link_device", [&] { return srb12_rollout_link_device(c12, 1, &k.b12, &k.sim12, pl, mv, sz, ag, nullptr, nullptr, 1, nullptr); }},
    };
    for (const auto &call : calls) report(call.first, k.name, call.second());
}

}  // namespace

int main()
{
    static double table[8];                // a table that is "there" (never read)
    std::vector<Case> cases;
    {
        Case k; k.name = "null context";
        cases.push_back(k);
        k.name = "null context, no structs"; k.with_mv = k.with_sz = k.with_ag = k.with_pl = false;
        cases.push_back(k);
    }
    {
        Case k; k.name = "batch struct_size"; k.b.struct_size -= 4; k.b12.struct_size -= 4;
        cases.push_back(k);
    }
    { Case k; k.name = "sim struct_size"; k.sim.struct_size += 8; k.sim12.struct_size += 8; cases.push_back(k); }
    { Case k; k.name = "srb12_plans struct_size"; k.pl.struct_size += 8; cases.push_back(k); }
    { Case k; k.name = "srb_moving struct_size"; k.mv.struct_size += 8; cases.push_back(k); }
    { Case k; k.name = "srb_sizes struct_size"; k.sz.struct_size += 8; cases.push_back(k); }
    { Case k; k.name = "srb_agent_sizes struct_size"; k.ag.struct_size += 8; cases.push_back(k); }
    { Case k; k.name = "horizon_selection without obs_vel"; k.mv.horizon_selection = 1; cases.push_back(k); }
    { Case k; k.name = "horizon_selection = 2"; k.mv.horizon_selection = 2; k.mv.obs_vel = table; cases.push_back(k); }
    {
        Case k; k.name = "obs_vel with obstacles_version"; k.mv.obs_vel = table;
        k.b.obstacles_version = 1; k.b12.obstacles_version = 1;
        cases.push_back(k);
    }
    { Case k; k.name = "obs_vel without srb_moving.obstacles"; k.mv.obs_vel = table; cases.push_back(k); }
    { Case k; k.name = "obs clearance_selection without obs_eps"; k.sz.clearance_selection = 1; cases.push_back(k); }
    { Case k; k.name = "nbr clearance_selection without agent_rad"; k.ag.clearance_selection = 1; cases.push_back(k); }
    { Case k; k.name = "agent_rad without a neighbour table"; k.ag.agent_rad = table; cases.push_back(k); }
    { Case k; k.name = "collide_cycle without agent_body"; static int cc[2]; k.ag.collide_cycle = cc; cases.push_back(k); }
    { Case k; k.name = "plan_selection without nbr_plan"; k.pl.plan_selection = 1; cases.push_back(k); }
    for (Case &k : cases) run_case(k);
    if (failures) std::fprintf(stderr, "%d call(s) were not refused\n", failures);
    return failures ? 1 : 0;
}
