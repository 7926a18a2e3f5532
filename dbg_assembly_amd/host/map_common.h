// map_common.h -- what bin/map_reads and bin/map_pair share on top of cli_common.h: the reference's option variables, its contig
// file format (link_scaffold/map_func.cpp:81-116), the mapper on the GPU (MAP section of include/dbgk.h), a batch of reads on
// its way to it and the formatting of one alignment; and, with DBGK_TEXT=device, what the route shares on which the text of a reads
// file never becomes strings: parsed, mapped, its rows composed and (with DBGK_GZ=device) deflated where they lie on the device.
#pragma once
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>
#include <cstdio>
#include <sstream>

#include "cli_common.h"
#include "text_window.h"

static int KmerSize = 31;
static double MinMapIdentity = 0.97;
static int SeedKmerNum = 5;
static int MinReadLen = 250;
static int MinCtgLen = 125;
static int Input_file_format = 1;
static string Output_prefix = "./";

static const uint64_t BatchReads = 1 << 20;   // reads per device batch
static const uint64_t BatchBases = 256 << 20; // ... or this many bases, whichever comes first

// read_contig_file (map_func.cpp:81-116): the id is the first token behind '>', sequences may span lines, a record
// without sequence in front of another header is dropped, the last record is always pushed
static void read_contig_file(const string &contig_seq_file, vector<string> &contig_ids, vector<string> &contig_seqs)
{
	ifstream infile(contig_seq_file.c_str());
	if (!infile) cerr << "fail to open input file " << contig_seq_file << endl;
	string id, seq_str, line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '>') {
			if (seq_str.size() > 0) {
				contig_ids.push_back(id);
				contig_seqs.push_back(seq_str);
			}
			vector<string> vec_line;
			split(line, vec_line, "> \t");
			id = vec_line.empty() ? string() : vec_line[0];
			seq_str.clear();
		} else if (line.size() > 0) {
			seq_str += line;
		}
	}
	contig_ids.push_back(id);
	contig_seqs.push_back(seq_str);
}

// the read id both programs print: first token of the header, "-" + the second one when there is one
static string make_read_id(const string &head, const char *delim)
{
	vector<string> vec_head;
	split(head, vec_head, delim);
	if (vec_head.empty()) return string();
	return vec_head.size() > 1 ? vec_head[0] + "-" + vec_head[1] : vec_head[0];
}

static const char *HeaderOne = "#read_id\tread_length\talign_read_start\talign_read_end\tcontig_id\tcontig_length\talign_contig_start\talign_contig_end\talign_direct\talign_identity%";
static const char *HeaderTwo = "\tread_id\tread_length\talign2_read_start\talign2_read_end\tcontig2_id\tcontig2_length\talign2_contig_start\talign2_contig_end\talign2_direct\talign2_identity%";

// the contigs as the programs hold them (short ones emptied, main of both programs) and the mapper that owns their index
struct Contigs {
	vector<string> ids, seqs;
	dbgk_map *mapper = nullptr;
	dbgk_maprow *rows = nullptr; // DBGK_TEXT=device: the rows of the hits, composed on the device (ROWS section of include/dbgk.h)

	void load(const string &file, int second_alignment)
	{
		read_contig_file(file, ids, seqs);
		uint64_t total_contig_num = 0, total_contig_len = 0;
		for (size_t i = 0; i < seqs.size(); i++) {
			if (seqs[i].size() >= (size_t)MinCtgLen) {
				total_contig_num++;
				total_contig_len += seqs[i].size();
			} else {
				seqs[i] = "";
			}
		}
		cerr << "\nInput contig sequence number: " << total_contig_num << endl;
		cerr << "Total contig sequence length: " << total_contig_len << endl;
		dbgk_map_params p{KmerSize, SeedKmerNum, MinReadLen, second_alignment, MinMapIdentity};
		int rc = dbgk_map_create(&p, 0, &mapper);
		if (rc) die("dbgk_map_create", rc);
		string bases;
		vector<uint64_t> offsets;
		concat(seqs, bases, offsets);
		rc = dbgk_map_set_contigs(mapper, bases.data(), offsets.data(), seqs.size());
		if (rc) die("dbgk_map_set_contigs", rc);
		cerr << "Build the kmer hash finished" << endl;
	}
	// DBGK_TEXT=device: the row writer of the program (mode DBGK_MAPROW_*, the delimiter set of its read ids) with the contig table every
	// row prints from: the ids, and the sizes as load() left them
	void rows_on_device(int mode, const char *delims)
	{
		int rc = dbgk_maprow_create(mode, delims, MinReadLen, 0, &rows);
		if (rc) die("dbgk_maprow_create", rc);
		string names;
		vector<uint64_t> offsets;
		concat(ids, names, offsets);
		vector<uint32_t> lengths(seqs.size());
		for (size_t i = 0; i < seqs.size(); i++) lengths[i] = (uint32_t)seqs[i].size();
		rc = dbgk_maprow_set_contigs(rows, names.data(), offsets.data(), lengths.data(), seqs.size());
		if (rc) die("dbgk_maprow_set_contigs", rc);
	}
	~Contigs()
	{
		if (rows) dbgk_maprow_destroy(rows);
		if (mapper) dbgk_map_destroy(mapper);
	}

	// one alignment as both programs print it; the identity is the reference's float expression (map_func.cpp:298)
	void row(ostream &o, const string &read_id, size_t read_len, const dbgk_map_hit &h) const
	{
		float identity = 1.0 - (float)h.mismatches / h.align_len;
		o << read_id << "\t" << read_len << "\t" << h.read_start << "\t" << h.read_end << "\t" << ids[h.contig] << "\t" << seqs[h.contig].size()
		  << "\t" << h.contig_start << "\t" << h.contig_end << "\t" << (char)h.direct << "\t" << identity * 100 << "%";
	}
};

// a batch of reads on its way to the device
struct ReadBatch {
	string bases;
	vector<uint64_t> offsets = vector<uint64_t>(1, 0);
	vector<dbgk_map_hit> hits;
	void add(const string &read)
	{
		bases += read;
		offsets.push_back(bases.size());
	}
	size_t size() const { return offsets.size() - 1; }
	bool full() const { return size() >= BatchReads || bases.size() >= BatchBases; }
	void map(dbgk_map *m)
	{
		hits.resize(2 * size() + 2);
		const int rc = dbgk_map_reads(m, bases.data(), offsets.data(), size(), hits.data());
		if (rc) die("dbgk_map_reads", rc);
	}
	void clear()
	{
		bases.clear();
		offsets.assign(1, 0);
	}
};

static void make_output_dir()
{
	if (mkdir(Output_prefix.c_str(), 0777) != 0 && errno != EEXIST) cerr << "fail to create " << Output_prefix << endl;
}

static string base_name(const string &path)
{
	const size_t pos = path.find_last_of('/');
	return pos == string::npos ? path : path.substr(pos + 1);
}

// ---- DBGK_TEXT=device -----------------------------------------------------------------------------------------------------------
// One reads file on its way through the parser, window by window (text_window.h): dbgk_parse_chunk without a quality plane (the two
// FASTQ lines behind the read are passed over unseen, as the host loops pass them), the batch left where dbgk_map_reads_device_keep and
// dbgk_maprow_rows_device read it.
struct ParsedFile {
	TextWindows in;
	dbgk_parse *parser = nullptr;
	dbgk_parse_info pi{};
	dbgk_maprow_side side{}; // the batch of the current window on the device (pi.n_records > 0)
	uint64_t n_bases = 0;
	double ms_parse = 0;
	explicit ParsedFile(const string &path) : in(path)
	{
		if (!in.ok()) cerr << "fail to open input file " << path << endl;
		const int rc = dbgk_parse_create(Input_file_format == 1 ? 1 : 2, 0, 0, &parser);
		if (rc) die("dbgk_parse_create", rc);
	}
	ParsedFile(const ParsedFile &) = delete;
	ParsedFile &operator=(const ParsedFile &) = delete;
	~ParsedFile() { if (parser) dbgk_parse_destroy(parser); }

	// the next window, parsed; false once the file has ended
	bool next()
	{
		if (!in.ok() || !in.next()) return false;
		int rc = dbgk_parse_chunk(parser, in.text(), in.n_text, in.last ? 1 : 0, &pi);
		if (rc) die("dbgk_parse_chunk", rc);
		ms_parse += pi.ms_lines + pi.ms_states + pi.ms_scan + pi.ms_gather;
		side = dbgk_maprow_side{};
		n_bases = 0;
		if (pi.n_records) {
			const char *d_quals;
			uint64_t n_reads;
			rc = dbgk_parse_device(parser, &side.bases, &d_quals, &side.offsets, &n_reads, &n_bases);
			if (rc) die("dbgk_parse_device", rc);
			rc = dbgk_parse_recs_device(parser, &side.recs);
			if (rc) die("dbgk_parse_recs_device", rc);
			rc = dbgk_parse_text_device(parser, &side.text, &side.n_text);
			if (rc) die("dbgk_parse_text_device", rc);
		}
		return true;
	}

	// the first n reads of the batch mapped, their hits left on the device and taken over as side `s` of the row writer
	void map_into(const Contigs &ctg, int s, uint64_t n)
	{
		int rc = dbgk_map_reads_device_keep(ctg.mapper, side.bases, side.offsets, n, n_bases, pi.max_len);
		if (rc) die("dbgk_map_reads_device_keep", rc);
		rc = dbgk_maprow_take_hits(ctg.rows, s, ctg.mapper);
		if (rc) die("dbgk_maprow_take_hits", rc);
	}

	// What the host loop needs of the first n records, for the one batch whose rows the device cannot print (an identity that needs
	// an exponent): the header lines out of the window's text, the reads, and the hits, mapped once more into host memory.
	void to_host(const Contigs &ctg, uint64_t n, vector<string> &heads, string &bases, vector<uint64_t> &offsets, vector<dbgk_map_hit> &hits)
	{
		vector<dbgk_parse_rec> recs(pi.n_records);
		vector<uint64_t> all(pi.n_records + 1);
		bases.resize(n_bases);
		int rc = dbgk_parse_results(parser, bases.data(), nullptr, all.data(), recs.data());
		if (rc) die("dbgk_parse_results", rc);
		offsets.assign(all.begin(), all.begin() + n + 1);
		heads.resize(n);
		for (uint64_t i = 0; i < n; i++) heads[i].assign(in.text() + recs[i].head_pos, recs[i].head_len);
		hits.resize(2 * n + 2);
		rc = dbgk_map_reads_device(ctg.mapper, side.bases, side.offsets, n, n_bases, pi.max_len, hits.data());
		if (rc) die("dbgk_map_reads_device", rc);
	}
};

// the rows of a batch are composed by the host loop although the device could: a test hook, so that the route of an unprintable
// identity is reached without an alignment of 2^24 bases
static bool rows_forced_to_host()
{
	const char *h = dbgk_hook("rows_on_host");
	return h && atoi(h) > 0;
}
