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
    bool any_parent = false;  // the one-taxon form: a child of the root, or the base's node wherever it hangs
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


// the manifest's lines, each checked on its own; by_id: external id -> index in lines
int read_lines(const char *path, std::vector<Line> &lines, std::map<uint64_t, size_t> &by_id, std::string &err) {
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
    return NH_OK;
}

// The tree of the lines, on top of the nodes of `base` where there is one, numbered as every tree here is.  A line whose taxid
// the base holds adds its files to that node (the base's name stays).
int number_tree(const char *path, std::vector<Line> &lines, const std::map<uint64_t, size_t> &by_id, const BaseTaxo *base,
                std::vector<TaxaNode> &nodes, std::vector<uint32_t> *remap, std::string &err) {
    nodes.clear();
    std::map<uint64_t, uint32_t> in_base;  // external id -> internal id of the base
    if (base)
        for (uint32_t i = 1; i < base->taxid.size(); i++) in_base[base->taxid[i]] = i;
    size_t added = 0;
    for (const auto &kv : by_id) {
        const Line &L = lines[kv.second];
        const auto b = in_base.find(L.taxid);
        if (b == in_base.end()) {
            added++;
            continue;
        }
        const uint64_t want = base->taxid[base->parent[b->second]];
        if (!L.any_parent && L.parent != want)
            return fail(err, NH_EINVAL, path, L.no, "taxid " + std::to_string(L.taxid) + " is in the base database under the parent " + std::to_string(want) +
                        ", not under " + std::to_string(L.parent));
    }
    if (base && base->taxid.size() - 1 + added > TAXA_MAX_NODES)
        return fail(err, NH_EINVAL, path, 0, "the base database's " + std::to_string(base->taxid.size() - 1) + " nodes and the " + std::to_string(added) +
                    " added are more than " + std::to_string(TAXA_MAX_NODES) + " nodes");
    // children of every node, in ascending external id (by_id is ordered)
    // (a child is a line, index + 1, or a node of the base, -(internal id); a taxid that is both is the base's node with the line's files)
    std::map<uint64_t, std::map<uint64_t, long>> kids;
    for (const auto &kv : by_id) {
        const Line &L = lines[kv.second];
        if (in_base.count(L.taxid)) continue;
        if (L.parent != 1 && !by_id.count(L.parent) && !in_base.count(L.parent))
            return fail(err, NH_EINVAL, path, L.no, "the parent taxid " + std::to_string(L.parent) + " is neither 1 (the root) nor a line of the manifest" +
                        (base ? " nor a taxon of the base database" : ""));
        kids[L.parent][L.taxid] = (long)kv.second + 1;
    }
    if (base)
        for (uint32_t i = 2; i < base->taxid.size(); i++) kids[base->taxid[base->parent[i]]][base->taxid[i]] = -(long)i;
    nodes.resize(2);
    nodes[1].taxid = 1;
    nodes[1].name = base ? base->name[1] : "root";
    if (base) nodes[1].rank = base->rank[1];
    if (remap) remap->assign(base ? base->taxid.size() : 0, 0);
    if (remap && base) (*remap)[1] = 1;
    std::vector<char> placed(lines.size(), 0);
    for (size_t i = 1; i < nodes.size(); i++) {  // breadth first: nodes grows while it is walked
        const auto k = kids.find(nodes[i].taxid);
        if (k == kids.end()) continue;
        nodes[i].first_child = (uint32_t)nodes.size();
        nodes[i].children = (uint32_t)k->second.size();
        for (const auto &kid : k->second) {
            TaxaNode n;
            n.taxid = kid.first;
            n.parent = (uint32_t)i;
            long li = kid.second;
            if (li < 0) {
                n.name = base->name[-li];
                n.rank = base->rank[-li];
                if (remap) (*remap)[-li] = (uint32_t)nodes.size();
                const auto again = by_id.find(kid.first);
                li = again == by_id.end() ? 0 : (long)again->second + 1;
            } else {
                n.name = std::move(lines[li - 1].name);
            }
            if (li > 0) {
                Line &L = lines[li - 1];
                placed[li - 1] = 1;
                n.line = L.no;
                n.files = std::move(L.files);
            }
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

}  // namespace

int parse_taxa(const char *path, std::vector<TaxaNode> &nodes, std::string &err) {
    nodes.clear();
    std::vector<Line> lines;
    std::map<uint64_t, size_t> by_id;
    const int rc = read_lines(path, lines, by_id, err);
    return rc ? rc : number_tree(path, lines, by_id, nullptr, nodes, nullptr, err);
}

int merge_taxa(const char *path, const BaseTaxo &base, std::vector<TaxaNode> &nodes, std::vector<uint32_t> &remap, std::string &err) {
    nodes.clear();
    std::vector<Line> lines;
    std::map<uint64_t, size_t> by_id;
    const int rc = read_lines(path, lines, by_id, err);
    return rc ? rc : number_tree(path, lines, by_id, &base, nodes, &remap, err);
}

int merge_taxon(uint64_t taxid, const std::string &name, const std::vector<std::string> &files, const BaseTaxo &base, std::vector<TaxaNode> &nodes,
                std::vector<uint32_t> &remap, std::string &err) {
    std::vector<Line> lines(1);
    lines[0].taxid = taxid, lines[0].parent = 1, lines[0].name = name, lines[0].files = files, lines[0].any_parent = true;
    std::map<uint64_t, size_t> by_id;
    by_id[taxid] = 0;
    return number_tree("the added taxon", lines, by_id, &base, nodes, &remap, err);
}

int read_base_taxo(const char *path, BaseTaxo &t, std::string &err) {
    auto bad = [&](const std::string &what) {
        err = std::string("nh_extend_db: ") + path + ": " + what;
        return (int)NH_EDB;
    };
    std::string img;
    {
        FILE *f = fopen(path, "rb");
        if (!f) {
            err = std::string("nh_extend_db: cannot read ") + path + ": " + strerror(errno);
            return NH_EIO;
        }
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) img.append(buf, n);
        fclose(f);
    }
    if (img.size() < 32 || memcmp(img.data(), "K2TAXDAT", 8) != 0) return bad("not a kraken2 taxonomy (bad magic)");
    uint64_t hdr[3];
    memcpy(hdr, img.data() + 8, 24);
    const uint64_t n = hdr[0];
    if (n < 2 || n > (1ull << 32) || hdr[1] > img.size() || hdr[2] > img.size() || 32 + n * 56 + hdr[1] + hdr[2] > img.size())
        return bad("truncated: " + std::to_string(img.size()) + " bytes do not hold the " + std::to_string(n) + " nodes and the string tables of its header");
    if (n - 1 > TAXA_MAX_NODES)
        return (err = std::string("nh_extend_db: ") + path + ": the base database has " + std::to_string(n - 1) + " nodes, more than " +
                      std::to_string(TAXA_MAX_NODES) + " nodes"), (int)NH_EINVAL;
    const char *names = img.data() + 32 + n * 56, *ranks = names + hdr[1];
    t.parent.assign(n, 0), t.taxid.assign(n, 0), t.name.assign(n, std::string()), t.rank.assign(n, std::string());
    std::map<uint64_t, uint64_t> seen;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t r[7];
        memcpy(r, img.data() + 32 + i * 56, 56);
        if (i >= 2 && (r[0] == 0 || r[0] >= i)) return bad("node " + std::to_string(i) + " has the parent " + std::to_string(r[0]) + ", which does not lie below it");
        if (r[3] >= hdr[1] && hdr[1]) return bad("node " + std::to_string(i) + ": its name lies outside the name table");
        if (r[4] >= hdr[2] && hdr[2]) return bad("node " + std::to_string(i) + ": its rank lies outside the rank table");
        t.parent[i] = i >= 2 ? (uint32_t)r[0] : 0;
        t.taxid[i] = r[5];
        if (hdr[1]) t.name[i].assign(names + r[3], strnlen(names + r[3], hdr[1] - r[3]));
        if (hdr[2]) t.rank[i].assign(ranks + r[4], strnlen(ranks + r[4], hdr[2] - r[4]));
        if (i >= 1 && !seen.emplace(r[5], i).second)
            return bad("the external id " + std::to_string(r[5]) + " appears twice (nodes " + std::to_string(seen[r[5]]) + " and " + std::to_string(i) + ")");
    }
    if (t.taxid[1] != 1) return bad("its root has the external id " + std::to_string(t.taxid[1]) + ", not 1");
    return NH_OK;
}

}  // namespace nh
