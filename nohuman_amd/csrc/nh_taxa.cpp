// nh_taxa.cpp -- parser of the taxa manifest (nh_taxa.h).  Host only.
#include "nh_taxa.h"

#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>

#include "nohuman_engine.h"

namespace nh {
namespace {

struct Line {
    uint32_t no = 0;
    uint64_t taxid = 0, parent = 0;
    std::string name;
    std::vector<std::string> files;
};

// decimal digits only, no sign, no overflow
bool parse_id(const std::string &s, uint64_t &v) {
    if (s.empty() || s.size() > 20) return false;
    v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        const uint64_t d = (uint64_t)(c - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    return true;
}

int fail(std::string &err, int code, const char *path, uint32_t line, const std::string &what) {
    char where[64] = "";
    if (line) snprintf(where, sizeof where, " line %u", line);
    err = std::string("nh_build_db: ") + path + where + ": " + what;
    return code;
}

}  // namespace

int parse_taxa(const char *path, std::vector<TaxaNode> &nodes, std::string &err) {
    nodes.clear();
    std::string text;
    {
        FILE *f = fopen(path, "rb");
        if (!f) return fail(err, NH_EIO, path, 0, std::string("cannot read the taxa manifest: ") + strerror(errno));
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) return fail(err, NH_EIO, path, 0, "cannot read the taxa manifest");
    }
    std::string dir = path;
    const size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);

    std::vector<Line> lines;
    std::map<uint64_t, size_t> by_id;    // external id -> index in lines
    std::map<std::string, uint32_t> seen_file;  // real path -> line
    uint32_t no = 0;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        std::string ln = text.substr(p, e - p);
        p = e + 1;
        no++;
        if (!ln.empty() && ln.back() == '\r') ln.pop_back();
        if (ln.empty() || ln[0] == '#') continue;
        std::vector<std::string> f;
        for (size_t a = 0;;) {
            const size_t t = ln.find('\t', a);
            f.push_back(ln.substr(a, t == std::string::npos ? std::string::npos : t - a));
            if (t == std::string::npos) break;
            a = t + 1;
        }
        if (f.size() < 3) return fail(err, NH_EINVAL, path, no, "fewer than three tab-separated fields (taxid, parent taxid, name)");
        Line L;
        L.no = no;
        if (!parse_id(f[0], L.taxid)) return fail(err, NH_EINVAL, path, no, "the taxid '" + f[0] + "' is not a number");
        if (L.taxid == 0) return fail(err, NH_EINVAL, path, no, "taxid 0 is no taxon");
        if (L.taxid == 1) return fail(err, NH_EINVAL, path, no, "taxid 1 is the root of the taxonomy, which is implicit and never a line");
        if (!parse_id(f[1], L.parent)) return fail(err, NH_EINVAL, path, no, "the parent taxid '" + f[1] + "' is not a number");
        if (f[2].empty()) return fail(err, NH_EINVAL, path, no, "the name is empty");
        L.name = f[2];
        const auto dup = by_id.find(L.taxid);
        if (dup != by_id.end())
            return fail(err, NH_EINVAL, path, no, "taxid " + f[0] + " appears twice (first on line " + std::to_string(lines[dup->second].no) + ")");
        for (size_t i = 3; i < f.size(); i++) {
            if (f[i].empty()) continue;  // (a trailing tab)
            const std::string full = f[i][0] == '/' ? f[i] : dir + f[i];
            char real[PATH_MAX];
            if (!realpath(full.c_str(), real))
                return fail(err, NH_EIO, path, no, "cannot read the FASTA file " + full + ": " + strerror(errno));
            const auto ins = seen_file.emplace(real, no);
            if (!ins.second)
                return fail(err, NH_EINVAL, path, no, "the FASTA file " + full + " is given twice (first on line " + std::to_string(ins.first->second) + ")");
            L.files.push_back(full);
        }
        if (lines.size() >= TAXA_MAX_NODES - 1)
            return fail(err, NH_EINVAL, path, no, "more than " + std::to_string(TAXA_MAX_NODES - 1) + " taxa");
        by_id[L.taxid] = lines.size();
        lines.push_back(std::move(L));
    }
    if (seen_file.empty()) return fail(err, NH_EINVAL, path, 0, "no FASTA file in the whole manifest");
    // children of every node, in ascending external id (by_id is ordered)
    std::map<uint64_t, std::vector<size_t>> kids;
    for (const auto &kv : by_id) {
        const Line &L = lines[kv.second];
        if (L.parent != 1 && !by_id.count(L.parent))
            return fail(err, NH_EINVAL, path, L.no, "the parent taxid " + std::to_string(L.parent) + " is neither 1 (the root) nor a line of the manifest");
        kids[L.parent].push_back(kv.second);
    }
    nodes.resize(2);
    nodes[1].taxid = 1;
    nodes[1].name = "root";
    std::vector<char> placed(lines.size(), 0);
    for (size_t i = 1; i < nodes.size(); i++) {  // breadth first: nodes grows while it is walked
        const auto k = kids.find(nodes[i].taxid);
        if (k == kids.end()) continue;
        nodes[i].first_child = (uint32_t)nodes.size();
        nodes[i].children = (uint32_t)k->second.size();
        for (size_t li : k->second) {
            Line &L = lines[li];
            placed[li] = 1;
            TaxaNode n;
            n.taxid = L.taxid;
            n.parent = (uint32_t)i;
            n.line = L.no;
            n.name = std::move(L.name);
            n.files = std::move(L.files);
            nodes.push_back(std::move(n));
        }
    }
    // every parent is a line or the root, so a line that the walk from the root did not reach lies on a cycle or below one
    for (size_t li = 0; li < lines.size(); li++)
        if (!placed[li]) {
            nodes.clear();
            return fail(err, NH_EINVAL, path, lines[li].no, "taxid " + std::to_string(lines[li].taxid) + " does not descend from the root: its parents form a cycle");
        }
    return NH_OK;
}

}  // namespace nh
